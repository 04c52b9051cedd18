"""
Weight generation on the device: the wrappers of the library's geometry entry
points (``include/remap_hip.h``) -- conservative overlaps, nearest points,
point location in triangles and quads, widened cells, areas and fractions,
the pieces of second-order and patch-recovery maps.  ``weights.py`` builds
mapping files from them.

:mod:`pyremap_amd.engine` loads the library and re-exports the public names
below (``engine.nearest_points`` ...), which is how the package calls them;
this module is imported by it and looks the library up through it.
"""
import ctypes
import numbers

import numpy as np

from pyremap_amd import engine
from pyremap_amd._abi import (_OverlapGeom, _OverlapGrid, _OverlapMesh,
                              _OverlapPieces, _OverlapSide)
from pyremap_amd.engine import _check, _gpu_ms, _ptr, _stream_ptr, _torch

#: the largest k of nearest_k_points (REMAP_NEAREST_K_MAX)
NEAREST_K_MAX = 16


# ---------------------------------------------------------------------------
# what the wrappers share: the argument check, the call behind a workspace
# ---------------------------------------------------------------------------

def _patch_args(torch, specs):
    """Every ``(name, tensor, dtype, trailing shape)`` of ``specs`` is a
    contiguous tensor of that dtype and shape ``(n,) + trailing`` on one HIP
    device, or a ``ValueError`` that names the argument.  A fifth item names
    the leading axes where they are not the one ``n``.  Returns the
    device."""
    for name, t, dtype, tail, *lead in specs:
        lead = lead[0] if lead else ('n',)
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or \
                t.dim() != len(lead) + len(tail) or \
                tuple(t.shape[len(lead):]) != tail or not t.is_contiguous():
            kind = 'int32' if dtype == torch.int32 else 'float64'
            shape = '(' + ', '.join(str(k) for k in lead + tail) + ')' \
                if tail else '(n,)'
            raise ValueError(
                f'{name}: expected a contiguous {shape} {kind} tensor on a '
                f'HIP device')
    devices = {s[1].device for s in specs}
    if len(devices) != 1:
        where = ', '.join(f'{s[0]} on {s[1].device}' for s in specs)
        raise ValueError(f'{where}: expected one device')
    return specs[0][1].device


def _checked(lib, rc, what):
    if rc == -1:     # REMAP_ERR_ARG
        raise ValueError(lib.remap_last_error().decode('utf-8', 'replace'))
    _check(rc, what)


def _behind_workspace(lib, name, dev, sizes, args, timing, phases=(),
                      arg_errors=False):
    """
    ``remap_<name>_workspace(*sizes, &bytes)``, a workspace of that size on
    ``dev``, then ``remap_<name>(*args, workspace, bytes, stream)`` on the
    current stream of ``dev``, its GPU time going to ``timing``
    (:func:`engine._gpu_ms`).  With ``phases``, three names, the call goes
    through ``remap_<name>_timed`` and ``timing`` also receives
    ``<phase>_ms`` of each.  ``arg_errors``: the library's ``REMAP_ERR_ARG``
    is a ``ValueError`` (:func:`_checked`).
    """
    torch = _torch()
    what = 'remap_' + name
    check = (lambda rc, what: _checked(lib, rc, what)) if arg_errors \
        else _check
    with torch.cuda.device(dev):
        stream = _stream_ptr(dev)
        nbytes = ctypes.c_size_t()
        check(getattr(lib, what + '_workspace')(*sizes, ctypes.byref(nbytes)),
              what + '_workspace')
        ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
        behind = (_ptr(ws), nbytes.value)
        if phases:
            what += '_timed'
            ms = (ctypes.c_float * len(phases))()
            behind += (ms,)
        with _gpu_ms(torch, timing):
            check(getattr(lib, what)(*args, *behind, stream), what)
        if phases:
            timing.update((p + '_ms', float(v)) for p, v in zip(phases, ms))
        # the workspace's memory returns to torch's allocator, which keeps it
        # for this stream: later work on the stream is ordered behind the call
        del ws


# ---------------------------------------------------------------------------
# conservative overlaps: what the four remap_overlap_* calls share
# ---------------------------------------------------------------------------

def _mesh_struct(torch, arrays, keep):
    """The ``remap_overlap_mesh`` of ``(verticesOnCell, nEdgesOnCell,
    latVertex, lonVertex)``; the converted tensors its pointers look into
    join ``keep``, which has to outlive the call."""
    voc = arrays[0].to(torch.int32).contiguous()
    noc = arrays[1].to(torch.int32).contiguous()
    lat_v = arrays[2].to(torch.float64).contiguous()
    lon_v = arrays[3].to(torch.float64).contiguous()
    keep.extend((voc, noc, lat_v, lon_v))
    return _OverlapMesh(voc.shape[0], lat_v.numel(), voc.shape[1], 0,
                        voc.data_ptr(), noc.data_ptr(), lat_v.data_ptr(),
                        lon_v.data_ptr())


def _overlap(kind, dev, sides, n_a, n_b, flag, n_dst, timing, counter_words=0,
             b_padded=True, arg_errors=False, phases=()):
    """
    ``remap_overlap_<kind>_sizes``, the workspace and the outputs, then
    ``remap_overlap_<kind>`` on the current stream of ``dev``: ``sides`` are
    the call's leading structs (one geometry, or sides a and b, of ``n_a``
    and ``n_b`` cells; the caller keeps the tensors behind them alive),
    ``flag`` its direction argument and ``n_dst`` the number of destination
    cells that follows from it.  ``counter_words``: the int64 words of the
    counter ``_sizes`` takes (0: it takes none).  ``b_padded=False``: the
    b-area array has exactly ``n_b`` elements.  ``arg_errors``: the library's
    ``REMAP_ERR_ARG`` is a ``ValueError``.  ``phases``: with ``timing`` the
    call goes through ``remap_overlap_<kind>_timed``, which reports these.

    Returns ``(dst, src, A, frac_b, a_area, b_area)`` cut to their lengths;
    ``timing`` receives ``n_pairs``, ``ms`` and the phases.
    """
    torch = _torch()
    lib = engine.load_library()
    what = f'remap_overlap_{kind}'

    def check(rc, name):
        if arg_errors and rc == -1:     # REMAP_ERR_ARG
            raise ValueError(
                f'{name}: ' +
                lib.remap_last_error().decode('utf-8', 'replace'))
        _check(rc, name)

    def empty(n, dtype=torch.float64):
        # (never empty: the C side wants every output pointer, even for a
        # mesh without cells)
        return torch.empty(max(n, 1), dtype=dtype, device=dev)
    sides = [ctypes.byref(s) for s in sides]
    with torch.cuda.device(dev):
        stream = _stream_ptr(dev)
        counter = []
        if counter_words:
            words = torch.zeros(counter_words, dtype=torch.int64, device=dev)
            counter = [_ptr(words)]
        n_pairs = ctypes.c_int64()
        nbytes = ctypes.c_size_t()
        check(getattr(lib, what + '_sizes')(
            *sides, *counter, ctypes.byref(n_pairs), ctypes.byref(nbytes),
            stream), what + '_sizes')
        n = n_pairs.value
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        dst, src, A = empty(n, torch.int32), empty(n, torch.int32), empty(n)
        a_area = empty(n_a)
        b_area = empty(n_b) if b_padded else \
            torch.empty(n_b, dtype=torch.float64, device=dev)
        frac_b = empty(n_dst)
        n_entries = ctypes.c_int64()
        args = (*sides, 1 if flag else 0, n, _ptr(ws), nbytes.value,
                _ptr(dst), _ptr(src), _ptr(A), _ptr(frac_b), _ptr(a_area),
                _ptr(b_area), ctypes.byref(n_entries))
        if phases and timing is not None:
            what += '_timed'
            ms = (ctypes.c_float * len(phases))()
            args += (ms,)
        with _gpu_ms(torch, timing):
            check(getattr(lib, what)(*args, stream), what)
        if timing is not None:
            timing['n_pairs'] = n
            if phases:
                timing.update(zip(phases, (float(x) for x in ms)))
        # (as in nearest_points: torch's allocator keeps the workspace for
        # this stream, so later work is ordered behind the call)
        del ws
        m = n_entries.value
    return (dst[:m], src[:m], A[:m], frac_b[:n_dst], a_area[:n_a],
            b_area[:n_b])


# ---------------------------------------------------------------------------
# conservative overlaps: MPAS cell mesh <-> lat-lon grid
# ---------------------------------------------------------------------------

def overlap_latlon(vertices_on_cell, n_edges_on_cell, lat_vertex, lon_vertex,
                   lat_corner, lon_corner, lat_slack, dst_is_mesh,
                   timing=None):
    """
    The overlap areas between the cells of an MPAS mesh (``verticesOnCell``
    1-based, ``nEdgesOnCell``, ``latVertex`` / ``lonVertex`` in radians) and
    the cells of a lat-lon grid (corner axes in radians; cell ``j * n_lon +
    i``), through ``remap_overlap_latlon`` (``include/remap_hip.h``).  All
    tensors on one HIP device; ``lat_slack``: the grid's great-circle bulge
    (radians).

    Returns ``(dst, src, A, frac_b, mesh_area, grid_area)``: 0-based int32
    indices and float64 areas (steradians) of the entries sorted by
    ``(dst, src)`` -- the mesh is the destination when ``dst_is_mesh`` --
    ``frac_b`` per destination cell, and both sets of polygon areas.
    ``timing``: a dict that receives ``n_pairs`` and the GPU ``ms`` of the
    overlap call (events on the stream).
    """
    torch = engine.require_gpu()
    dev = vertices_on_cell.device
    voc = vertices_on_cell.to(torch.int32).contiguous()
    noc = n_edges_on_cell.to(torch.int32).contiguous()
    lat_v = lat_vertex.to(torch.float64).contiguous()
    lon_v = lon_vertex.to(torch.float64).contiguous()
    lat_c = lat_corner.to(torch.float64).contiguous()
    lon_c = lon_corner.to(torch.float64).contiguous()
    n_cells, max_edges = voc.shape
    n_lat, n_lon = lat_c.numel() - 1, lon_c.numel() - 1
    geom = _OverlapGeom(n_cells, lat_v.numel(), n_lat, n_lon, max_edges, 0,
                        float(lat_slack), voc.data_ptr(), noc.data_ptr(),
                        lat_v.data_ptr(), lon_v.data_ptr(), lat_c.data_ptr(),
                        lon_c.data_ptr())
    n_grid = n_lat * n_lon
    return _overlap('latlon', dev, (geom,), n_cells, n_grid, dst_is_mesh,
                    n_cells if dst_is_mesh else n_grid, timing,
                    counter_words=2, b_padded=False)


# ---------------------------------------------------------------------------
# conservative overlaps: MPAS cell mesh <-> MPAS cell mesh
# (overlap_meshes, like overlap_pieces and overlap_grids below, builds its two
# side structs and leaves the rest to _overlap)
# ---------------------------------------------------------------------------

def overlap_meshes(mesh_a, mesh_b, dst_is_b, timing=None):
    """
    The overlap areas between the cells of two MPAS meshes, each given as
    ``(verticesOnCell 1-based, nEdgesOnCell, latVertex, lonVertex)`` (radians)
    tensors on one HIP device, through ``remap_overlap_meshes``
    (``include/remap_hip.h``).  Mesh a's polygons are clipped by mesh b's,
    which must be convex; both directions use the same overlap list.

    Returns ``(dst, src, A, frac_b, a_area, b_area)``: 0-based int32 indices
    and float64 areas (steradians) of the entries sorted by ``(dst, src)``
    -- mesh b is the destination when ``dst_is_b`` -- ``frac_b`` per
    destination cell, and both sets of polygon areas.  ``timing``: a dict
    that receives ``n_pairs`` (candidates) and the GPU ``ms`` of the overlap
    call (events on the stream).
    """
    torch = engine.require_gpu()
    keep = []
    ga = _mesh_struct(torch, mesh_a, keep)
    gb = _mesh_struct(torch, mesh_b, keep)
    n_a, n_b = ga.n_cells, gb.n_cells
    return _overlap('meshes', mesh_a[0].device, (ga, gb), n_a, n_b, dst_is_b,
                    n_b if dst_is_b else n_a, timing, counter_words=4)


# ---------------------------------------------------------------------------
# conservative overlaps between cells that come in convex pieces
# ---------------------------------------------------------------------------

#: the phases ``remap_overlap_pieces_timed`` reports, in order
PIECES_PHASES = ('prep_ms', 'pairs_ms', 'clip_ms', 'sort_ms', 'merge_ms')


def overlap_pieces(pieces_a, pieces_b, dst_is_b, timing=None):
    """
    The overlap areas between the cells of two polygon soups, each cell given
    as one or more convex pieces, through ``remap_overlap_pieces``
    (``include/remap_hip.h``).  A side is ``(verticesOnCell 1-based,
    nEdgesOnCell, latVertex, lonVertex, parent, n_parents)``: the first four
    describe the PIECES as :func:`overlap_meshes` takes a mesh, ``parent``
    (int32, 0-based, non-decreasing, every cell at least once) says which
    cell a piece belongs to -- ``None``: piece k is cell k, and ``n_parents``
    is the number of pieces.  Side a's pieces are clipped by side b's, which
    must be convex.

    Returns ``(dst, src, A, frac_b, a_area, b_area)`` as
    :func:`overlap_meshes` does, in cells: the areas of the piece pairs of a
    pair of cells added in ascending (dst piece, src piece) order.  With
    ``parent=None`` on both sides the bytes are those of
    :func:`overlap_meshes`.  ``timing``: a dict that receives ``n_pairs``
    (candidate piece pairs), the GPU ``ms`` of the call and its phases
    (:data:`PIECES_PHASES`, the merge ``merge_ms``) from
    ``remap_overlap_pieces_timed``.

    A ``parent`` that decreases, leaves ``[0, n_parents)`` or skips a cell is
    a ``ValueError`` (the library's ``REMAP_ERR_ARG``).
    """
    torch = engine.require_gpu()
    dev = pieces_a[0].device
    keep = []

    def side(p):
        mesh = _mesh_struct(torch, p, keep)
        parent, n_parents = p[4], int(p[5])
        ptr = None
        if parent is not None:
            parent = parent.to(device=dev, dtype=torch.int32).contiguous()
            if parent.numel() != mesh.n_cells:
                raise ValueError(
                    f'overlap_pieces: {parent.numel()} parents for '
                    f'{mesh.n_cells} pieces')
            keep.append(parent)
            ptr = parent.data_ptr()
        return _OverlapPieces(mesh, n_parents, ptr)
    ga, gb = side(pieces_a), side(pieces_b)
    n_a, n_b = ga.n_parents, gb.n_parents
    return _overlap('pieces', dev, (ga, gb), n_a, n_b, dst_is_b,
                    n_b if dst_is_b else n_a, timing, counter_words=4,
                    arg_errors=True, phases=PIECES_PHASES)


# ---------------------------------------------------------------------------
# conservative overlaps with a structured 2-D grid on one side or both
# ---------------------------------------------------------------------------

def overlap_grids(side_a, side_b, dst_is_b, timing=None):
    """
    The overlap areas between the cells of two sides, at least one of them a
    structured 2-D grid, through ``remap_overlap_grids``
    (``include/remap_hip.h``).  A side is a grid ``(lat_corner, lon_corner)``
    -- two ``(ny + 1, nx + 1)`` tensors in radians, cell ``j * nx + i`` --
    or an MPAS mesh ``(verticesOnCell 1-based, nEdgesOnCell, latVertex,
    lonVertex)`` as in :func:`overlap_meshes`; all tensors on one HIP device.
    Side a's polygons are clipped by side b's, which must be convex; both
    directions use the same overlap list.

    Returns ``(dst, src, A, frac_b, a_area, b_area)`` as
    :func:`overlap_meshes` does -- side b is the destination when
    ``dst_is_b``.  ``timing``: a dict that receives ``n_pairs`` (candidates)
    and the GPU ``ms`` of the overlap call (events on the stream).
    """
    torch = engine.require_gpu()
    keep = []

    def side(arrays):
        if len(arrays) == 2:
            lat = arrays[0].to(torch.float64).contiguous()
            lon = arrays[1].to(torch.float64).contiguous()
            if lat.dim() != 2 or lat.shape != lon.shape or \
                    min(lat.shape) < 2:
                raise ValueError(
                    f'grid corners of shapes {tuple(lat.shape)} and '
                    f'{tuple(lon.shape)}: expected two (ny + 1, nx + 1) '
                    f'arrays')
            g = _OverlapGrid(lat.shape[0] - 1, lat.shape[1] - 1,
                             lat.data_ptr(), lon.data_ptr())
            keep.extend((lat, lon, g))
            return _OverlapSide(None, ctypes.pointer(g)), int(g.ny * g.nx)
        m = _mesh_struct(torch, arrays, keep)
        keep.append(m)
        return _OverlapSide(ctypes.pointer(m), None), int(m.n_cells)
    (ga, n_a), (gb, n_b) = side(side_a), side(side_b)
    return _overlap('grids', side_a[0].device, (ga, gb), n_a, n_b, dst_is_b,
                    n_b if dst_is_b else n_a, timing)


# ---------------------------------------------------------------------------
# nearest source point of every destination point (ESMF's neareststod)
# ---------------------------------------------------------------------------

def nearest_points(src_xyz, dst_xyz, timing=None, phases=False):
    """
    The index (0-based, ``int32``) of the source point nearest to every
    destination point, through ``remap_nearest`` (``include/remap_hip.h``):
    ``src_xyz (n_src, 3)`` and ``dst_xyz (n_dst, 3)`` are contiguous fp64
    tensors on one HIP device, finite.  Exact: the minimum of ``d2 = (dx*dx +
    dy*dy) + dz*dz`` in fp64 in that order, the lowest source index among
    equal ``d2``; two calls give identical bytes.  Asynchronous on the
    current stream.

    ``timing``: a dict that receives the GPU ``ms`` of the call (events on
    the stream).  With ``phases=True`` (measurements only: the library then
    waits for the walk before it returns) the call goes through
    ``remap_nearest_timed`` and the dict also receives ``sort_ms``,
    ``pyramid_ms`` and ``walk_ms``.
    """
    torch = engine.require_gpu()
    lib = engine.load_library()
    dev = _patch_args(torch, (('src_xyz', src_xyz, torch.float64, (3,)),
                              ('dst_xyz', dst_xyz, torch.float64, (3,))))
    n_src, n_dst = src_xyz.shape[0], dst_xyz.shape[0]
    if n_src < 1:
        raise ValueError('nearest_points needs at least one source point')
    if phases and timing is None:
        raise ValueError('phases=True needs a timing dict to fill')
    out = torch.empty(n_dst, dtype=torch.int32, device=dev)
    _behind_workspace(
        lib, 'nearest', dev, (n_src, n_dst),
        (_ptr(src_xyz), n_src, _ptr(dst_xyz), n_dst, _ptr(out)), timing,
        ('sort', 'pyramid', 'walk') if phases else ())
    return out


def nearest_k_points(src_xyz, dst_xyz, k, timing=None):
    """
    The ``k`` nearest source points of every destination point, through
    ``remap_nearest_k`` (``include/remap_hip.h``): ``(idx, d2)``, an
    ``int32`` and a ``float64`` tensor of shape ``(n_dst, k)``.  Row ``i``
    holds the ``min(k, n_src)`` sources that come first in ``(d2, index)``
    order, ascending, with ``d2`` as in :func:`nearest_points`; the slots
    behind them hold index -1 and ``d2`` = +inf.  The tensors are as for
    :func:`nearest_points`, ``k`` is 1 .. ``NEAREST_K_MAX``; exact, two calls
    give identical bytes, ``k = 1`` gives :func:`nearest_points`' indices.
    Asynchronous on the current stream.  ``timing``: a dict that receives
    the GPU ``ms`` of the call.
    """
    torch = engine.require_gpu()
    lib = engine.load_library()
    dev = _patch_args(torch, (('src_xyz', src_xyz, torch.float64, (3,)),
                              ('dst_xyz', dst_xyz, torch.float64, (3,))))
    n_src, n_dst = src_xyz.shape[0], dst_xyz.shape[0]
    if n_src < 1:
        raise ValueError('nearest_k_points needs at least one source point')
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or \
            not 1 <= k <= NEAREST_K_MAX:
        raise ValueError(f'k = {k!r}: expected an integer from 1 to '
                         f'{NEAREST_K_MAX}')
    k = int(k)
    idx = torch.empty((n_dst, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((n_dst, k), dtype=torch.float64, device=dev)
    _behind_workspace(
        lib, 'nearest_k', dev, (n_src, n_dst, k),
        (_ptr(src_xyz), n_src, _ptr(dst_xyz), n_dst, k, _ptr(idx), _ptr(d2)),
        timing)
    return idx, d2


# ---------------------------------------------------------------------------
# the triangle that holds every point (bilinear from an MPAS mesh)
# ---------------------------------------------------------------------------

def locate_in_triangles(xyz, tri, points, tol=1e-12, timing=None,
                        phases=False):
    """
    For every point the lowest-numbered spherical triangle that holds it and
    the weights of its three corners, through ``remap_locate``
    (``include/remap_hip.h`` has the definition): ``xyz (n_nodes, 3)`` and
    ``points (n_pts, 3)`` are contiguous fp64 tensors, ``tri (n_tri, 3)`` a
    contiguous int32 tensor of node ids, all on one HIP device; nodes and
    points are unit vectors.  Returns ``(found int32 (n_pts,), weights fp64
    (n_pts, 3))`` on that device: ``found`` is -1, and the weights zero, where
    no triangle holds the point.  Exact in fp64 (the barycentric coordinates
    of the point's central projection, a corner accepted down to ``-tol``);
    two calls give identical bytes.  Asynchronous on the current stream.

    ``timing``: a dict that receives the GPU ``ms`` of the call (events on
    the stream).  With ``phases=True`` (measurements only: the library then
    waits for the walk before it returns) the call goes through
    ``remap_locate_timed`` and the dict also receives ``sort_ms``,
    ``setup_ms`` and ``walk_ms``.
    """
    torch = engine.require_gpu()
    lib = engine.load_library()
    dev = _patch_args(torch, (('xyz', xyz, torch.float64, (3,)),
                              ('tri', tri, torch.int32, (3,)),
                              ('points', points, torch.float64, (3,))))
    n_nodes, n_tri, n_pts = xyz.shape[0], tri.shape[0], points.shape[0]
    if n_tri < 1 or n_nodes < 1:
        raise ValueError('locate_in_triangles needs at least one triangle '
                         'and one node')
    tol = float(tol)
    if not tol >= 0.0:
        raise ValueError(f'tol {tol}: expected a number >= 0')
    if phases and timing is None:
        raise ValueError('phases=True needs a timing dict to fill')
    found = torch.empty(n_pts, dtype=torch.int32, device=dev)
    weights = torch.empty((n_pts, 3), dtype=torch.float64, device=dev)
    _behind_workspace(
        lib, 'locate', dev, (n_nodes, n_tri, n_pts),
        (_ptr(xyz), n_nodes, _ptr(tri), n_tri, _ptr(points), n_pts, tol,
         _ptr(found), _ptr(weights)), timing,
        ('sort', 'setup', 'walk') if phases else ())
    return found, weights


# ---------------------------------------------------------------------------
# the quad of four cell centres that holds every point (bilinear from a grid
# given by 2-D latitude / longitude arrays)
# ---------------------------------------------------------------------------

def locate_in_quads(nodes, points, periodic=False, tol=1e-10, timing=None,
                    phases=False):
    """
    For every point the lowest-numbered quad of four neighbouring cell
    centres whose bilinear patch holds it, and the patch's weights of the
    four corners, through ``remap_quads`` (``include/remap_hip.h`` has the
    definition): ``nodes (ny, nx, 3)`` and ``points (n_pts, 3)`` are
    contiguous fp64 tensors of unit vectors on one HIP device, ``ny >= 2``
    and ``nx >= 2``; with ``periodic`` column ``nx - 1`` closes onto column
    0.  Quad ``k = j * nqx + i`` (``nqx = nx - 1 + periodic``) has the corners
    ``(j, i)``, ``(j, i1)``, ``(j + 1, i1)``, ``(j + 1, i)`` with ``i1 = (i +
    1) % nx``, the order of the weights.  Returns ``(found int32 (n_pts,),
    weights fp64 (n_pts, 4))`` on that device: ``found`` is -1, and the
    weights zero, where no quad holds the point.  Exact in fp64 (a Newton
    solve per point and quad with a stopping rule of its own, the patch
    coordinates accepted up to ``1 + tol``); two calls give identical bytes.
    Asynchronous on the current stream.

    ``timing``: a dict that receives the GPU ``ms`` of the call (events on
    the stream).  With ``phases=True`` (measurements only: the library then
    waits for the walk before it returns) the call goes through
    ``remap_quads_timed`` and the dict also receives ``sort_ms``,
    ``setup_ms`` and ``walk_ms``.
    """
    torch = engine.require_gpu()
    lib = engine.load_library()
    dev = _patch_args(torch, (
        ('nodes', nodes, torch.float64, (3,), ('ny', 'nx')),
        ('points', points, torch.float64, (3,))))
    ny, nx, n_pts = nodes.shape[0], nodes.shape[1], points.shape[0]
    if ny < 2 or nx < 2:
        raise ValueError(f'locate_in_quads needs at least 2 x 2 nodes, not '
                         f'{ny} x {nx}')
    periodic = 1 if periodic else 0
    tol = float(tol)
    if not tol >= 0.0:
        raise ValueError(f'tol {tol}: expected a number >= 0')
    if phases and timing is None:
        raise ValueError('phases=True needs a timing dict to fill')
    found = torch.empty(n_pts, dtype=torch.int32, device=dev)
    weights = torch.empty((n_pts, 4), dtype=torch.float64, device=dev)
    _behind_workspace(
        lib, 'quads', dev, (ny, nx, periodic, n_pts),
        (_ptr(nodes), ny, nx, periodic, _ptr(points), n_pts, tol,
         _ptr(found), _ptr(weights)), timing,
        ('sort', 'setup', 'walk') if phases else ())
    return found, weights


# ---------------------------------------------------------------------------
# cells widened about their centres (expand_dist / expand_factor)
# ---------------------------------------------------------------------------

def expand_cells(centre_lat, centre_lon, corner_lat, corner_lon, count,
                 expand_dist=None, expand_factor=None, timing=None):
    """
    The corners of every cell moved away from the cell's centre, through
    ``remap_expand_cells`` (``include/remap_hip.h`` has the definition and
    its three rules; :func:`pyremap_amd.weights.expand_cells` is the same
    statement in numpy): ``centre_lat`` / ``centre_lon`` ``(n,)``,
    ``corner_lat`` / ``corner_lon`` ``(n, width)`` fp64 tensors in radians
    and ``count (n,)`` integers, all on one HIP device.  ``expand_dist``
    (metres; ``None``: 0) and ``expand_factor`` (``None``: 1) are numbers or
    ``(n,)`` arrays / tensors, one value per cell.

    Returns ``(lat, lon)``, two new ``(n, width)`` fp64 tensors on that
    device; slots beyond ``count[i]`` hold copies.  Runs on the current
    stream and waits for it (the status is read back).  ``n = 0`` is legal.
    A NaN, a count outside ``[0, width]`` or a corner whose new distance
    ``factor * d + dist`` is not positive is a ``ValueError`` that names the
    first such cell (the library's ``REMAP_ERR_ARG``).  ``timing``: a dict
    that receives the GPU ``ms`` of the call (events on the stream).
    """
    torch = engine.require_gpu()
    lib = engine.load_library()
    if not torch.is_tensor(corner_lat) or not corner_lat.is_cuda or \
            corner_lat.dim() != 2 or corner_lat.shape[1] < 1:
        raise ValueError('corner_lat: expected an (n, width) tensor on a HIP '
                         'device, width >= 1')
    dev = corner_lat.device
    n, width = corner_lat.shape

    def f64(name, t, shape):
        if not torch.is_tensor(t) or t.device != dev or \
                tuple(t.shape) != shape:
            raise ValueError(
                f'{name}: expected a tensor of shape {shape} on {dev}')
        return t.to(torch.float64).contiguous()

    def per_cell(name, value, default):
        if value is None:
            value = default
        if not torch.is_tensor(value):
            value = torch.as_tensor(np.asarray(value, dtype=np.float64))
        value = value.to(device=dev, dtype=torch.float64).contiguous()
        if value.dim() == 0:
            return value.reshape(1), 0
        if tuple(value.shape) != (n,):
            raise ValueError(
                f'{name} of shape {tuple(value.shape)}: expected a number '
                f'or one value for each of the {n} cells')
        # (a one-cell array has one value either way)
        return (value, 1) if n > 0 else (value.new_zeros(1), 0)
    corner_lat = f64('corner_lat', corner_lat, (n, width))
    corner_lon = f64('corner_lon', corner_lon, (n, width))
    centre_lat = f64('centre_lat', centre_lat, (n,))
    centre_lon = f64('centre_lon', centre_lon, (n,))
    if not torch.is_tensor(count) or count.device != dev or \
            tuple(count.shape) != (n,) or count.dtype.is_floating_point:
        raise ValueError(f'count: expected {n} integers on {dev}')
    count = count.to(torch.int32).contiguous()
    dist, dist_stride = per_cell('expand_dist', expand_dist, 0.0)
    factor, factor_stride = per_cell('expand_factor', expand_factor, 1.0)
    with torch.cuda.device(dev):
        stream = _stream_ptr(dev)
        out_lat = torch.empty_like(corner_lat)
        out_lon = torch.empty_like(corner_lon)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        with _gpu_ms(torch, timing):
            rc = lib.remap_expand_cells(
                n, width, _ptr(centre_lat), _ptr(centre_lon),
                _ptr(corner_lat), _ptr(corner_lon), _ptr(count), _ptr(dist),
                dist_stride, _ptr(factor), factor_stride, _ptr(out_lat),
                _ptr(out_lon), _ptr(status), stream)
            if rc == -1:     # REMAP_ERR_ARG
                raise ValueError(
                    lib.remap_last_error().decode('utf-8', 'replace'))
            _check(rc, 'remap_expand_cells')
    return out_lat, out_lon


# ---------------------------------------------------------------------------
# what a complete mapping file says about its grids: areas and frac_a
# ---------------------------------------------------------------------------

#: REMAP_CELL_AREAS_MAX_WIDTH
CELL_AREAS_MAX_WIDTH = 32


def cell_areas(corner_lat, corner_lon, count, timing=None):
    """
    The area in steradians of every cell given in SCRIP layout, through
    ``remap_cell_areas`` (``include/remap_hip.h`` has the definition;
    :func:`pyremap_amd.weights.cell_areas` is the same statement in numpy):
    ``corner_lat`` / ``corner_lon`` ``(n, width)`` fp64 tensors in radians
    and ``count (n,)`` integers on one HIP device, the first ``count[i]``
    corners of row i the cell's great-circle polygon.  Returns a new ``(n,)``
    fp64 tensor.  Runs on the current stream and waits for it.  A count
    outside ``[0, width]`` is a ``ValueError`` that names the first such
    cell (the library's ``REMAP_ERR_ARG``).  ``timing``: a dict that
    receives the GPU ``ms`` of the call.
    """
    torch = engine.require_gpu()
    lib = engine.load_library()
    if not torch.is_tensor(corner_lat) or not corner_lat.is_cuda or \
            corner_lat.dim() != 2 or corner_lat.shape[1] < 1:
        raise ValueError('corner_lat: expected an (n, width) tensor on a HIP '
                         'device, width >= 1')
    dev = corner_lat.device
    n, width = corner_lat.shape
    if not torch.is_tensor(corner_lon) or corner_lon.device != dev or \
            tuple(corner_lon.shape) != (n, width):
        raise ValueError(f'corner_lon: expected a tensor of shape '
                         f'{(n, width)} on {dev}')
    if not torch.is_tensor(count) or count.device != dev or \
            tuple(count.shape) != (n,) or count.dtype.is_floating_point:
        raise ValueError(f'count: expected {n} integers on {dev}')
    corner_lat = corner_lat.to(torch.float64).contiguous()
    corner_lon = corner_lon.to(torch.float64).contiguous()
    count = count.to(torch.int32).contiguous()
    with torch.cuda.device(dev):
        stream = _stream_ptr(dev)
        area = torch.empty(n, dtype=torch.float64, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        with _gpu_ms(torch, timing):
            rc = lib.remap_cell_areas(n, width, _ptr(corner_lat),
                                      _ptr(corner_lon), _ptr(count),
                                      _ptr(area), _ptr(status), stream)
            if rc == -1:     # REMAP_ERR_ARG
                raise ValueError(
                    lib.remap_last_error().decode('utf-8', 'replace'))
            _check(rc, 'remap_cell_areas')
    return area


def column_fractions(col, value, n_cols, denom=None, clamp=False,
                     index_base=0, timing=None):
    """
    ``out[j] = sum of value[k] over col[k] - index_base == j``, added in
    ascending k -- ``np.bincount(col, weights=value, minlength=n_cols)``, bit
    for bit -- then divided by ``denom[j]`` when ``denom`` is given and cut
    to at most 1 when ``clamp`` is set; a column without entries is 0.
    Through ``remap_column_fractions`` (``include/remap_hip.h``;
    :func:`pyremap_amd.weights.column_fractions` is the numpy statement):
    ``col`` integers and ``value`` fp64, 1-D tensors of one length on one
    HIP device, ``denom`` ``(n_cols,)`` fp64 there.  Returns a new
    ``(n_cols,)`` fp64 tensor; two calls give the same bytes.  An entry whose
    column is outside ``[0, n_cols)`` is a ``ValueError`` (the count is read
    back, which waits for the stream).  ``timing``: a dict that receives the
    GPU ``ms`` of the call.
    """
    torch = engine.require_gpu()
    lib = engine.load_library()
    if not torch.is_tensor(value) or not value.is_cuda or value.dim() != 1:
        raise ValueError('value: expected a 1-D tensor on a HIP device')
    dev = value.device
    n = value.shape[0]
    n_cols = int(n_cols)
    if not torch.is_tensor(col) or col.device != dev or \
            tuple(col.shape) != (n,) or col.dtype.is_floating_point:
        raise ValueError(f'col: expected {n} integers on {dev}')
    if n and (int(col.max()) > 2 ** 31 - 1 or int(col.min()) < -2 ** 31):
        raise ValueError('col: beyond int32')
    if denom is not None and (
            not torch.is_tensor(denom) or denom.device != dev or
            tuple(denom.shape) != (n_cols,)):
        raise ValueError(f'denom: expected a tensor of shape ({n_cols},) on '
                         f'{dev}')
    col = col.to(torch.int32).contiguous()
    value = value.to(torch.float64).contiguous()
    if denom is not None:
        denom = denom.to(torch.float64).contiguous()
    out = torch.empty(n_cols, dtype=torch.float64, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    _behind_workspace(
        lib, 'column_fractions', dev, (n,),
        (n, n_cols, _ptr(col), int(index_base), _ptr(value), _ptr(denom),
         1 if clamp else 0, _ptr(out), _ptr(bad)), timing)
    n_bad = int(bad.item())
    if n_bad:
        raise ValueError(f'{n_bad} entries name a column outside '
                         f'[0, {n_cols})')
    return out


# ---------------------------------------------------------------------------
# second-order conservative maps: moments, gradient stencils, the assembly
# ---------------------------------------------------------------------------

#: REMAP_OVERLAP_MAX_EDGES
OVERLAP_MAX_EDGES = 10


def _scrip_cells(torch, name, corner_lat, corner_lon, count, dev=None):
    """``(lat, lon, count)`` of one side in SCRIP layout, checked the way
    :func:`cell_areas` checks its own and made fp64 / int32, contiguous."""
    if not torch.is_tensor(corner_lat) or not corner_lat.is_cuda or \
            corner_lat.dim() != 2 or corner_lat.shape[1] < 1 or \
            (dev is not None and corner_lat.device != dev):
        raise ValueError(
            f'{name}corner_lat: expected an (n, width) tensor on '
            f'{"a HIP device" if dev is None else dev}, width >= 1')
    dev = corner_lat.device
    n, width = corner_lat.shape
    if not torch.is_tensor(corner_lon) or corner_lon.device != dev or \
            tuple(corner_lon.shape) != (n, width):
        raise ValueError(f'{name}corner_lon: expected a tensor of shape '
                         f'{(n, width)} on {dev}')
    if not torch.is_tensor(count) or count.device != dev or \
            tuple(count.shape) != (n,) or count.dtype.is_floating_point:
        raise ValueError(f'{name}count: expected {n} integers on {dev}')
    return (corner_lat.to(torch.float64).contiguous(),
            corner_lon.to(torch.float64).contiguous(),
            count.to(torch.int32).contiguous())


def _f64(torch, name, t, shape, dev):
    if not torch.is_tensor(t) or t.device != dev or \
            tuple(t.shape) != shape or not t.dtype.is_floating_point:
        raise ValueError(f'{name}: expected a floating-point tensor of shape '
                         f'{shape} on {dev}')
    return t.to(torch.float64).contiguous()


def _i32(torch, name, t, shape, dev):
    if not torch.is_tensor(t) or t.device != dev or \
            tuple(t.shape) != shape or t.dtype.is_floating_point:
        raise ValueError(f'{name}: expected integers of shape {shape} on '
                         f'{dev}')
    return t.to(torch.int32).contiguous()


def cell_moments(corner_lat, corner_lon, count, timing=None):
    """
    The first moment ``M = integral of r dA`` (unit sphere) of every cell
    given in SCRIP layout, through ``remap_cell_moments``
    (``include/remap_hip.h`` has the definition;
    :func:`pyremap_amd.weights.cell_moments` is the same statement in
    numpy): the arguments and the errors of :func:`cell_areas`.  Returns a
    new ``(n, 3)`` fp64 tensor.  Runs on the current stream and waits for
    it.  ``timing``: a dict that receives the GPU ``ms`` of the call.
    """
    torch = engine.require_gpu()
    lib = engine.load_library()
    corner_lat, corner_lon, count = _scrip_cells(torch, '', corner_lat,
                                                 corner_lon, count)
    dev = corner_lat.device
    n, width = corner_lat.shape
    with torch.cuda.device(dev):
        stream = _stream_ptr(dev)
        moment = torch.empty((n, 3), dtype=torch.float64, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        with _gpu_ms(torch, timing):
            _checked(lib, lib.remap_cell_moments(
                n, width, _ptr(corner_lat), _ptr(corner_lon), _ptr(count),
                _ptr(moment), _ptr(status), stream), 'remap_cell_moments')
    return moment


def overlap_moments(dst, src, area, src_cells, src_area, src_moment,
                    dst_cells, timing=None):
    """
    ``M_ij``, the first moment of (source cell ``src[e]`` n destination cell
    ``dst[e]``) for every first-order entry, through
    ``remap_overlap_moments`` (``include/remap_hip.h``): ``dst`` / ``src``
    0-based integers and ``area`` (``A_ij``) as an ``overlap_*`` call returns
    them, ``src_cells`` / ``dst_cells`` the two sides as ``(corner_lat,
    corner_lon, count)`` in SCRIP layout (radians, width at most
    ``OVERLAP_MAX_EDGES``: an :class:`EngineError` otherwise), ``src_area``
    ``(n_src,)`` and ``src_moment`` ``(n_src, 3)``; everything on one HIP
    device.  An entry whose clip leaves fewer than 3 corners gets ``A_ij *
    M_j / A_j``.  Returns a new ``(n_entries, 3)`` fp64 tensor.  Runs on the
    current stream and waits for it.  ``ValueError``: a wrong shape, dtype
    or device, an entry outside its side, a count outside ``[0, width]``.
    """
    torch = engine.require_gpu()
    lib = engine.load_library()
    s_lat, s_lon, s_count = _scrip_cells(torch, 'source ', *src_cells)
    dev = s_lat.device
    d_lat, d_lon, d_count = _scrip_cells(torch, 'destination ', *dst_cells,
                                         dev=dev)
    n_src, w_src = s_lat.shape
    n_dst, w_dst = d_lat.shape
    if not torch.is_tensor(area) or area.dim() != 1:
        raise ValueError('area: expected a 1-D tensor')
    n = area.shape[0]
    area = _f64(torch, 'area', area, (n,), dev)
    dst = _i32(torch, 'dst', dst, (n,), dev)
    src = _i32(torch, 'src', src, (n,), dev)
    src_area = _f64(torch, 'src_area', src_area, (n_src,), dev)
    src_moment = _f64(torch, 'src_moment', src_moment, (n_src, 3), dev)
    moment = torch.empty((n, 3), dtype=torch.float64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    _behind_workspace(
        lib, 'overlap_moments', dev, (n_src, w_src, n_dst, w_dst),
        (n, _ptr(dst), _ptr(src), _ptr(area), n_src, w_src, _ptr(s_lat),
         _ptr(s_lon), _ptr(s_count), _ptr(src_area), _ptr(src_moment), n_dst,
         w_dst, _ptr(d_lat), _ptr(d_lon), _ptr(d_count), _ptr(moment),
         _ptr(status)), timing, arg_errors=True)
    return moment


def gradient_stencils(nbr, count, centroid, timing=None):
    """
    The gradient coefficients of every cell over its edge neighbours,
    through ``remap_gradient_stencils`` (``include/remap_hip.h``;
    :func:`pyremap_amd.weights.gradient_stencils` is the numpy statement):
    ``nbr`` ``(n, width)`` integers (-1: no cell across that edge),
    ``count`` ``(n,)`` integers and ``centroid`` ``(n, 3)`` unit vectors on
    one HIP device, width at most ``OVERLAP_MAX_EDGES``.  Returns ``(coef
    (n, width + 1, 3) fp64, has (n,) int32)``: slot 0 the cell itself, slot
    ``1 + t`` neighbour ``t``; all 0 where ``has`` is 0.  Runs on the
    current stream and waits for it.
    """
    torch = engine.require_gpu()
    lib = engine.load_library()
    if not torch.is_tensor(nbr) or not nbr.is_cuda or nbr.dim() != 2 or \
            nbr.shape[1] < 1 or nbr.dtype.is_floating_point:
        raise ValueError('nbr: expected (n, width) integers on a HIP '
                         'device, width >= 1')
    dev = nbr.device
    n, width = nbr.shape
    nbr = nbr.to(torch.int32).contiguous()
    count = _i32(torch, 'count', count, (n,), dev)
    centroid = _f64(torch, 'centroid', centroid, (n, 3), dev)
    with torch.cuda.device(dev):
        stream = _stream_ptr(dev)
        coef = torch.empty((n, width + 1, 3), dtype=torch.float64,
                           device=dev)
        has = torch.empty(n, dtype=torch.int32, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        with _gpu_ms(torch, timing):
            _checked(lib, lib.remap_gradient_stencils(
                n, width, _ptr(nbr), _ptr(count), _ptr(centroid), _ptr(coef),
                _ptr(has), _ptr(status), stream), 'remap_gradient_stencils')
    return coef, has


def conserve2nd_assemble(dst, src, area, moment, nbr, count, coef, has,
                         src_area, src_moment, dst_area, timing=None):
    """
    The second-order map from its pieces, through
    ``remap_conserve2nd_sizes`` / ``remap_conserve2nd_assemble``
    (``include/remap_hip.h``; :func:`pyremap_amd.weights.second_order_entries`
    is the numpy statement): the first-order entries ``dst`` / ``src`` /
    ``area`` with their moments ``(n_entries, 3)``, the source's ``nbr (n_src,
    width)``, ``count``, ``coef (n_src, width + 1, 3)`` and ``has``,
    ``src_area``, ``src_moment (n_src, 3)`` and ``dst_area (n_dst,)``, all on
    one HIP device.  Returns ``(row, col, S)``, new tensors (int32 0-based,
    fp64) sorted by ``(row, col)`` and unique; zero sums are kept.  Two
    calls give the same bytes.  Runs on the current stream and waits for it
    twice (the triple count, the entry count).  ``timing`` receives the GPU
    ``ms`` of the assembly call.
    """
    torch = engine.require_gpu()
    lib = engine.load_library()
    if not torch.is_tensor(area) or not area.is_cuda or area.dim() != 1:
        raise ValueError('area: expected a 1-D tensor on a HIP device')
    dev = area.device
    n = area.shape[0]
    if not torch.is_tensor(nbr) or nbr.dim() != 2 or nbr.shape[1] < 1:
        raise ValueError('nbr: expected (n_src, width) integers, width >= 1')
    n_src, width = nbr.shape
    if not torch.is_tensor(dst_area) or dst_area.dim() != 1:
        raise ValueError('dst_area: expected a 1-D tensor')
    n_dst = dst_area.shape[0]
    area = _f64(torch, 'area', area, (n,), dev)
    dst = _i32(torch, 'dst', dst, (n,), dev)
    src = _i32(torch, 'src', src, (n,), dev)
    moment = _f64(torch, 'moment', moment, (n, 3), dev)
    nbr = _i32(torch, 'nbr', nbr, (n_src, width), dev)
    count = _i32(torch, 'count', count, (n_src,), dev)
    coef = _f64(torch, 'coef', coef, (n_src, width + 1, 3), dev)
    has = _i32(torch, 'has', has, (n_src,), dev)
    src_area = _f64(torch, 'src_area', src_area, (n_src,), dev)
    src_moment = _f64(torch, 'src_moment', src_moment, (n_src, 3), dev)
    dst_area = _f64(torch, 'dst_area', dst_area, (n_dst,), dev)
    with torch.cuda.device(dev):
        stream = _stream_ptr(dev)
        counters = torch.zeros(2, dtype=torch.int64, device=dev)
        capacity = ctypes.c_int64(0)
        need = ctypes.c_size_t(0)
        _checked(lib, lib.remap_conserve2nd_sizes(
            n, _ptr(src), n_src, width, _ptr(count), _ptr(has),
            _ptr(counters), ctypes.byref(capacity), ctypes.byref(need),
            stream), 'remap_conserve2nd_sizes')
        cap = capacity.value
        workspace = torch.empty(max(need.value, 1), dtype=torch.uint8,
                                device=dev)
        row = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        col = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        S = torch.empty(max(cap, 1), dtype=torch.float64, device=dev)
        n_out = ctypes.c_int64(0)
        with _gpu_ms(torch, timing):
            _checked(lib, lib.remap_conserve2nd_assemble(
                n, _ptr(dst), _ptr(src), _ptr(area), _ptr(moment), n_src,
                width, _ptr(nbr), _ptr(count), _ptr(coef), _ptr(has),
                _ptr(src_area), _ptr(src_moment), n_dst, _ptr(dst_area), cap,
                _ptr(workspace), need.value, _ptr(row), _ptr(col), _ptr(S),
                _ptr(counters), ctypes.byref(n_out), stream),
                'remap_conserve2nd_assemble')
        del workspace
    k = n_out.value
    return row[:k], col[:k], S[:k]


# ---------------------------------------------------------------------------
# patch-recovery maps: one-rings, a quadratic per node, the rows
# ---------------------------------------------------------------------------

#: REMAP_PATCH_MAX_RING, REMAP_PATCH_FIT_WIDTH
PATCH_MAX_RING = 16
PATCH_FIT_WIDTH = 22


def _same_length(specs):
    """Every ``(name, tensor, n, of)`` has ``n`` rows (one per ``of``)."""
    for name, t, n, of in specs:
        if t.shape[0] != n:
            raise ValueError(f'{name}: {t.shape[0]} rows, expected one for '
                             f'each of the {n} {of}')


def node_rings(tri, n_nodes, timing=None):
    """
    The one-ring of every node of the triangles ``tri (n_tri, 3)`` (a
    contiguous int32 tensor of node ids below ``n_nodes`` on a HIP device),
    through ``remap_node_rings`` (``include/remap_hip.h`` has the
    definition; :func:`pyremap_amd.weights.node_rings` is the numpy
    statement).  Returns ``(ring int32 (n_nodes, PATCH_MAX_RING), count
    int32 (n_nodes,))``: the distinct nodes that share a triangle with each
    node, ascending, padded with -1, and their true number (of which the
    lowest ``PATCH_MAX_RING`` are kept).  Two calls give identical bytes.
    Runs on the current stream and waits for it.  ``ValueError``: a triangle
    names a node outside ``[0, n_nodes)``.  ``timing``: a dict that receives
    the GPU ``ms`` of the call.
    """
    torch = engine.require_gpu()
    lib = engine.load_library()
    dev = _patch_args(torch, (('tri', tri, torch.int32, (3,)),))
    n_nodes = int(n_nodes)
    if n_nodes < 1:
        raise ValueError(f'n_nodes {n_nodes}: expected at least one node')
    n_tri = tri.shape[0]
    ring = torch.empty((n_nodes, PATCH_MAX_RING), dtype=torch.int32,
                       device=dev)
    count = torch.empty(n_nodes, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _behind_workspace(
        lib, 'node_rings', dev, (n_tri, n_nodes),
        (n_tri, _ptr(tri), n_nodes, _ptr(ring), _ptr(count), _ptr(status)),
        timing, arg_errors=True)
    return ring, count


def patch_fits(xyz, ring, count, timing=None):
    """
    The least-squares quadratic of every node over itself and its ring,
    through ``remap_patch_fits`` (``include/remap_hip.h``;
    :func:`pyremap_amd.weights.patch_fits` is the numpy statement): ``xyz
    (n, 3)`` fp64 unit vectors, ``ring (n, PATCH_MAX_RING)`` and ``count
    (n,)`` int32 as :func:`node_rings` returns them, contiguous, on one HIP
    device.  Returns ``(fit fp64 (n, PATCH_FIT_WIDTH), has int32 (n,))``:
    the scale ``h`` and the upper triangle of ``N^-1`` where the node has a
    patch, zeros where ``has`` is 0.  Runs on the current stream and waits
    for it.  ``timing``: a dict that receives the GPU ``ms`` of the call.
    """
    torch = engine.require_gpu()
    lib = engine.load_library()
    dev = _patch_args(torch, (
        ('xyz', xyz, torch.float64, (3,)),
        ('ring', ring, torch.int32, (PATCH_MAX_RING,)),
        ('count', count, torch.int32, ())))
    n = xyz.shape[0]
    if n < 1:
        raise ValueError('patch_fits needs at least one node')
    _same_length((('ring', ring, n, 'nodes'), ('count', count, n, 'nodes')))
    with torch.cuda.device(dev):
        stream = _stream_ptr(dev)
        fit = torch.empty((n, PATCH_FIT_WIDTH), dtype=torch.float64,
                          device=dev)
        has = torch.empty(n, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        with _gpu_ms(torch, timing):
            _checked(lib, lib.remap_patch_fits(
                n, _ptr(xyz), _ptr(ring), _ptr(count), _ptr(fit), _ptr(has),
                _ptr(status), stream), 'remap_patch_fits')
    return fit, has


def patch_rows(xyz, tri, ring, count, fit, has, found, w, points,
               timing=None):
    """
    The patch map's rows, through ``remap_patch_sizes`` /
    ``remap_patch_rows`` (``include/remap_hip.h``;
    :func:`pyremap_amd.weights.patch_entries` is the numpy statement):
    ``xyz``, ``tri`` and ``points`` as :func:`locate_in_triangles` takes
    them, ``found (n_pts,)`` / ``w (n_pts, 3)`` as it returns them, ``ring``
    / ``count`` of :func:`node_rings` and ``fit`` / ``has`` of
    :func:`patch_fits`; contiguous fp64 / int32 tensors on one HIP device.
    Returns ``(row, col, S)``, new tensors (int32 0-based, fp64) sorted by
    ``(row, col)`` and unique; zero sums are kept; a point with ``found =
    -1`` has no row.  A point whose triangle touches a node without a patch
    keeps its three located weights, bit for bit.  Two calls give the same
    bytes.  Runs on the current stream and waits for it twice (the entry
    count, the status).  ``timing`` receives the GPU ``ms`` of both passes.
    """
    torch = engine.require_gpu()
    lib = engine.load_library()
    dev = _patch_args(torch, (
        ('xyz', xyz, torch.float64, (3,)),
        ('tri', tri, torch.int32, (3,)),
        ('ring', ring, torch.int32, (PATCH_MAX_RING,)),
        ('count', count, torch.int32, ()),
        ('fit', fit, torch.float64, (PATCH_FIT_WIDTH,)),
        ('has', has, torch.int32, ()),
        ('found', found, torch.int32, ()),
        ('w', w, torch.float64, (3,)),
        ('points', points, torch.float64, (3,))))
    n, n_tri, n_pts = xyz.shape[0], tri.shape[0], points.shape[0]
    if n < 1:
        raise ValueError('patch_rows needs at least one node')
    _same_length((('ring', ring, n, 'nodes'), ('count', count, n, 'nodes'),
                  ('fit', fit, n, 'nodes'), ('has', has, n, 'nodes'),
                  ('found', found, n_pts, 'points'),
                  ('w', w, n_pts, 'points')))
    with torch.cuda.device(dev):
        stream = _stream_ptr(dev)
        need = ctypes.c_size_t(0)
        _checked(lib, lib.remap_patch_sizes_workspace(
            n_pts, ctypes.byref(need)), 'remap_patch_sizes_workspace')
        workspace = torch.empty(max(need.value, 1), dtype=torch.uint8,
                                device=dev)
        offsets = torch.empty(n_pts + 1, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        total = ctypes.c_int64(0)
        with _gpu_ms(torch, timing):
            _checked(lib, lib.remap_patch_sizes(
                n, _ptr(xyz), n_tri, _ptr(tri), _ptr(ring), _ptr(count),
                _ptr(has), n_pts, _ptr(found), _ptr(points), _ptr(offsets),
                ctypes.byref(total), _ptr(status), _ptr(workspace),
                need.value, stream), 'remap_patch_sizes')
            cap = total.value
            row = torch.empty(cap, dtype=torch.int32, device=dev)
            col = torch.empty(cap, dtype=torch.int32, device=dev)
            S = torch.empty(cap, dtype=torch.float64, device=dev)
            _checked(lib, lib.remap_patch_rows(
                n, _ptr(xyz), n_tri, _ptr(tri), _ptr(ring), _ptr(count),
                _ptr(fit), _ptr(has), n_pts, _ptr(found), _ptr(w),
                _ptr(points), _ptr(offsets), cap, _ptr(row), _ptr(col),
                _ptr(S), _ptr(status), stream), 'remap_patch_rows')
        del workspace
    return row, col, S
