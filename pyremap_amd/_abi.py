"""
The ctypes mirror of ``include/remap_hip.h``, stated once: its structs
(``STRUCTS``), the prototype of every entry point (``PROTOTYPES``) and
:func:`declare`, which sets them on a loaded library.  The header is the
contract and this file is written by hand; ``tests/test_host_cpu.py`` holds
the two together (every parameter's class, every member's offset).
"""
import ctypes
from ctypes import POINTER

#: REMAP_MODE_FILL_BEST / REMAP_MODE_FILL_MEAN: one pass of a creeping fill
#: (``pyremap_amd.engine`` holds the other modes by their numbers)
MODE_FILL_BEST = 20
MODE_FILL_MEAN = 21


class _CSR(ctypes.Structure):
    _fields_ = [
        ('n_rows', ctypes.c_int64),
        ('n_cols', ctypes.c_int64),
        ('nnz', ctypes.c_int64),
        ('rowptr', ctypes.c_void_p),
        ('col', ctypes.c_void_p),
        ('val', ctypes.c_void_p),
        ('max_row_nnz', ctypes.c_int64),
        ('csr_pad', ctypes.c_int64),
    ]


class _ApplyArgs(ctypes.Structure):
    _fields_ = [
        ('A', _CSR),
        ('row_begin', ctypes.c_int64),
        ('row_end', ctypes.c_int64),
        ('X', ctypes.c_void_p),
        ('x_dtype', ctypes.c_int32),
        ('mode', ctypes.c_int32),
        ('x_row_stride', ctypes.c_int64),
        ('x_batch_stride', ctypes.c_int64),
        ('Y', ctypes.c_void_p),
        ('y_row_stride', ctypes.c_int64),
        ('y_batch_stride', ctypes.c_int64),
        ('n_batch', ctypes.c_int64),
        ('k_inner', ctypes.c_int64),
        ('frac_b', ctypes.c_void_p),
        ('threshold', ctypes.c_double),
        ('mask_out', ctypes.c_void_p),
        ('row_order', ctypes.c_void_p),
        ('patch_ptr', ctypes.c_void_p),
        ('patch_ucol', ctypes.c_void_p),
        ('patch_rowptr', ctypes.c_void_p),
        ('patch_lidx', ctypes.c_void_p),
        ('patch_val', ctypes.c_void_p),
        ('patch_rows', ctypes.c_int32),
        ('patch_umax', ctypes.c_int32),
        ('patch_emax', ctypes.c_int32),
        ('patch_row_bytes', ctypes.c_int32),
        ('n_patches', ctypes.c_int64),
        ('group_meta', ctypes.c_void_p),
        ('group_col', ctypes.c_void_p),
        ('group_w', ctypes.c_void_p),
        ('group_mask', ctypes.c_void_p),
        ('group_rid', ctypes.c_void_p),
        ('group_frac', ctypes.c_void_p),
        ('n_groups', ctypes.c_int64),
        ('group_rows', ctypes.c_int32),
        ('group_reserved', ctypes.c_int32),
        ('gate', ctypes.c_void_p),
        ('gate_value', ctypes.c_int32),
        ('flags', ctypes.c_uint32),
        ('tune', ctypes.c_int32 * 8),
        ('x_src_fold', ctypes.c_int64),
        ('x_outer_stride', ctypes.c_int64),
        ('patch_ell_base', ctypes.c_void_p),
        ('strips', ctypes.c_void_p),
        ('share_meta', ctypes.c_void_p),
        ('share_col', ctypes.c_void_p),
        ('share_mask', ctypes.c_void_p),
        ('share_waves', ctypes.c_int32),
        ('share_reserved', ctypes.c_int32),
    ]


class _LimitArgs(ctypes.Structure):     # struct remap_limit_args
    _fields_ = [
        ('A', _CSR),
        ('row_begin', ctypes.c_int64),
        ('row_end', ctypes.c_int64),
        ('X', ctypes.c_void_p),
        ('x_dtype', ctypes.c_int32),
        ('x_row_stride', ctypes.c_int64),
        ('x_batch_stride', ctypes.c_int64),
        ('x_src_fold', ctypes.c_int64),
        ('x_outer_stride', ctypes.c_int64),
        ('Y', ctypes.c_void_p),
        ('y_row_stride', ctypes.c_int64),
        ('y_batch_stride', ctypes.c_int64),
        ('n_batch', ctypes.c_int64),
        ('k_inner', ctypes.c_int64),
        ('lo', ctypes.c_void_p),
        ('hi', ctypes.c_void_p),
    ]


class _SgsArgs(ctypes.Structure):       # struct remap_sgs_args
    _fields_ = [
        ('A', _CSR),
        ('row_begin', ctypes.c_int64),
        ('row_end', ctypes.c_int64),
        ('X', ctypes.c_void_p),
        ('x_dtype', ctypes.c_int32),
        ('x_row_stride', ctypes.c_int64),
        ('x_batch_stride', ctypes.c_int64),
        ('x_src_fold', ctypes.c_int64),
        ('x_outer_stride', ctypes.c_int64),
        ('F', ctypes.c_void_p),
        ('f_dtype', ctypes.c_int32),
        ('f_row_stride', ctypes.c_int64),
        ('f_batch_stride', ctypes.c_int64),
        ('f_inner_stride', ctypes.c_int64),
        ('f_outer_stride', ctypes.c_int64),
        ('Y', ctypes.c_void_p),
        ('y_row_stride', ctypes.c_int64),
        ('y_batch_stride', ctypes.c_int64),
        ('n_batch', ctypes.c_int64),
        ('k_inner', ctypes.c_int64),
        ('threshold', ctypes.c_double),
    ]


class _LevelsArgs(ctypes.Structure):    # struct remap_levels_args
    _fields_ = [
        ('A', _CSR),
        ('row_begin', ctypes.c_int64),
        ('row_end', ctypes.c_int64),
        ('X', ctypes.c_void_p),
        ('x_dtype', ctypes.c_int32),
        ('x_row_stride', ctypes.c_int64),
        ('x_batch_stride', ctypes.c_int64),
        ('x_src_fold', ctypes.c_int64),
        ('x_outer_stride', ctypes.c_int64),
        ('n_levels', ctypes.c_int64),
        ('Z', ctypes.c_void_p),
        ('z_dtype', ctypes.c_int32),
        ('z_row_stride', ctypes.c_int64),
        ('z_batch_stride', ctypes.c_int64),
        ('z_outer_stride', ctypes.c_int64),
        ('T', ctypes.c_void_p),
        ('Y', ctypes.c_void_p),
        ('y_row_stride', ctypes.c_int64),
        ('y_batch_stride', ctypes.c_int64),
        ('n_batch', ctypes.c_int64),
        ('k_inner', ctypes.c_int64),
        ('threshold', ctypes.c_double),
    ]


class _LayersArgs(ctypes.Structure):    # struct remap_layers_args
    _fields_ = [
        ('A', _CSR),
        ('row_begin', ctypes.c_int64),
        ('row_end', ctypes.c_int64),
        ('X', ctypes.c_void_p),
        ('x_dtype', ctypes.c_int32),
        ('x_row_stride', ctypes.c_int64),
        ('x_batch_stride', ctypes.c_int64),
        ('x_src_fold', ctypes.c_int64),
        ('x_outer_stride', ctypes.c_int64),
        ('n_levels', ctypes.c_int64),
        ('H', ctypes.c_void_p),
        ('h_dtype', ctypes.c_int32),
        ('h_row_stride', ctypes.c_int64),
        ('h_batch_stride', ctypes.c_int64),
        ('h_outer_stride', ctypes.c_int64),
        ('bounds', ctypes.c_void_p),
        ('Y', ctypes.c_void_p),
        ('y_row_stride', ctypes.c_int64),
        ('y_batch_stride', ctypes.c_int64),
        ('n_batch', ctypes.c_int64),
        ('k_inner', ctypes.c_int64),
        ('threshold', ctypes.c_double),
        ('reduce', ctypes.c_int32),
    ]


class _VectorArgs(ctypes.Structure):    # struct remap_vector_args
    _fields_ = [
        ('A', _CSR),
        ('row_begin', ctypes.c_int64),
        ('row_end', ctypes.c_int64),
        ('U', ctypes.c_void_p),
        ('V', ctypes.c_void_p),
        ('x_dtype', ctypes.c_int32),
        ('x_row_stride', ctypes.c_int64),
        ('x_batch_stride', ctypes.c_int64),
        ('x_src_fold', ctypes.c_int64),
        ('x_outer_stride', ctypes.c_int64),
        ('BA', ctypes.c_void_p),
        ('BB', ctypes.c_void_p),
        ('YU', ctypes.c_void_p),
        ('YV', ctypes.c_void_p),
        ('y_row_stride', ctypes.c_int64),
        ('y_batch_stride', ctypes.c_int64),
        ('n_batch', ctypes.c_int64),
        ('k_inner', ctypes.c_int64),
        ('threshold', ctypes.c_double),
    ]


class _Strips(ctypes.Structure):         # struct remap_strips
    _fields_ = [
        ('n_units', ctypes.c_int64),
        ('steps_per_unit', ctypes.c_int32),
        ('rows_per_wave', ctypes.c_int32),
        ('ring_slots', ctypes.c_int32),
        ('depth', ctypes.c_int32),
        ('meta_slot_bytes', ctypes.c_int32),
        ('waves', ctypes.c_int32),
        ('unit_steps', ctypes.c_void_p),
        ('arr_ptr', ctypes.c_void_p),
        ('arr_src', ctypes.c_void_p),
        ('arr_slot', ctypes.c_void_p),
        ('meta_ptr', ctypes.c_void_p),
        ('meta', ctypes.c_void_p),
    ]


class _Schedule(ctypes.Structure):
    _fields_ = [
        ('family', ctypes.c_int32),
        ('entry_rich', ctypes.c_int32),
        ('row_order', ctypes.c_void_p),
        ('patch_ptr', ctypes.c_void_p),
        ('patch_ucol', ctypes.c_void_p),
        ('patch_rowptr', ctypes.c_void_p),
        ('patch_lidx', ctypes.c_void_p),
        ('patch_val', ctypes.c_void_p),
        ('patch_rows', ctypes.c_int32),
        ('patch_umax', ctypes.c_int32),
        ('patch_emax', ctypes.c_int32),
        ('patch_row_bytes', ctypes.c_int32),
        ('n_patches', ctypes.c_int64),
        ('group_meta', ctypes.c_void_p),
        ('group_col', ctypes.c_void_p),
        ('group_w', ctypes.c_void_p),
        ('group_mask', ctypes.c_void_p),
        ('group_rid', ctypes.c_void_p),
        ('group_frac', ctypes.c_void_p),
        ('n_groups', ctypes.c_int64),
        ('group_rows', ctypes.c_int32),
        ('super_tile', ctypes.c_int32),
        ('tile_y', ctypes.c_int32),
        ('tile_x', ctypes.c_int32),
        ('ratio', ctypes.c_double),
        ('n_distinct', ctypes.c_int64),
        ('tune', (ctypes.c_int32 * 8) * 3),
        ('arena_used', ctypes.c_size_t),
        ('share_meta', ctypes.c_void_p),
        ('share_col', ctypes.c_void_p),
        ('share_mask', ctypes.c_void_p),
        ('share_waves', ctypes.c_int32),
        ('share_reserved', ctypes.c_int32),
        ('n_share_union', ctypes.c_int64),
    ]


class _PlanInfo(ctypes.Structure):     # struct remap_plan_info
    _fields_ = [
        ('n_a', ctypes.c_int64),
        ('n_b', ctypes.c_int64),
        ('nnz', ctypes.c_int64),
        ('max_row_nnz', ctypes.c_int64),
        ('family', ctypes.c_int32),
        ('group_rows', ctypes.c_int32),
        ('ratio', ctypes.c_double),
        ('device_bytes', ctypes.c_size_t),
        ('cell_patch_rows', ctypes.c_int32),
        ('reserved', ctypes.c_int32),
    ]


class _Field(ctypes.Structure):        # struct remap_field
    _fields_ = [
        ('X', ctypes.c_void_p),
        ('x_dtype', ctypes.c_int32),
        ('mode', ctypes.c_int32),
        ('n_batch', ctypes.c_int64),
        ('k_inner', ctypes.c_int64),
        ('x_row_stride', ctypes.c_int64),
        ('x_batch_stride', ctypes.c_int64),
        ('Y', ctypes.c_void_p),
        ('y_row_stride', ctypes.c_int64),
        ('y_batch_stride', ctypes.c_int64),
        ('threshold', ctypes.c_double),
        ('mask_out', ctypes.c_void_p),
        ('gate', ctypes.c_void_p),
        ('gate_value', ctypes.c_int32),
        ('flags', ctypes.c_uint32),
    ]


class _OverlapGeom(ctypes.Structure):  # struct remap_overlap_geom
    _fields_ = [('n_cells', ctypes.c_int64),
                ('n_vertices', ctypes.c_int64),
                ('n_lat', ctypes.c_int64),
                ('n_lon', ctypes.c_int64),
                ('max_edges', ctypes.c_int32),
                ('reserved', ctypes.c_int32),
                ('lat_slack', ctypes.c_double),
                ('vertices_on_cell', ctypes.c_void_p),
                ('n_edges_on_cell', ctypes.c_void_p),
                ('lat_vertex', ctypes.c_void_p),
                ('lon_vertex', ctypes.c_void_p),
                ('lat_corner', ctypes.c_void_p),
                ('lon_corner', ctypes.c_void_p)]


class _OverlapMesh(ctypes.Structure):  # struct remap_overlap_mesh
    _fields_ = [('n_cells', ctypes.c_int64),
                ('n_vertices', ctypes.c_int64),
                ('max_edges', ctypes.c_int32),
                ('reserved', ctypes.c_int32),
                ('vertices_on_cell', ctypes.c_void_p),
                ('n_edges_on_cell', ctypes.c_void_p),
                ('lat_vertex', ctypes.c_void_p),
                ('lon_vertex', ctypes.c_void_p)]


class _OverlapPieces(ctypes.Structure):  # struct remap_overlap_pieces
    _fields_ = [('mesh', _OverlapMesh),
                ('n_parents', ctypes.c_int64),
                ('parent', ctypes.c_void_p)]


class _OverlapGrid(ctypes.Structure):  # struct remap_overlap_grid
    _fields_ = [('ny', ctypes.c_int64),
                ('nx', ctypes.c_int64),
                ('lat_corner', ctypes.c_void_p),
                ('lon_corner', ctypes.c_void_p)]


class _OverlapSide(ctypes.Structure):  # struct remap_overlap_side
    _fields_ = [('mesh', ctypes.POINTER(_OverlapMesh)),
                ('grid', ctypes.POINTER(_OverlapGrid))]


#: the header's name of every struct -> its mirror
STRUCTS = {
    'remap_csr': _CSR,
    'remap_strips': _Strips,
    'remap_apply_args': _ApplyArgs,
    'remap_schedule': _Schedule,
    'remap_plan_info': _PlanInfo,
    'remap_field': _Field,
    'remap_overlap_geom': _OverlapGeom,
    'remap_overlap_mesh': _OverlapMesh,
    'remap_overlap_pieces': _OverlapPieces,
    'remap_overlap_grid': _OverlapGrid,
    'remap_overlap_side': _OverlapSide,
    'remap_limit_args': _LimitArgs,
    'remap_sgs_args': _SgsArgs,
    'remap_vector_args': _VectorArgs,
    'remap_levels_args': _LevelsArgs,
    'remap_layers_args': _LayersArgs,
}

# A parameter as the table below writes it.  P: any pointer that is passed as
# an address -- device memory, a stream, the opaque remap_plan; HOST_*: a
# pointer to host numbers that ctypes passes by reference or as an array; a
# pointer to one of the structs above is POINTER(its mirror).
P = ctypes.c_void_p
I32 = ctypes.c_int32            # int32_t and int
I64 = ctypes.c_int64
F64 = ctypes.c_double
SIZE = ctypes.c_size_t
HOST_SIZE = POINTER(ctypes.c_size_t)
HOST_I64 = POINTER(ctypes.c_int64)
HOST_F32 = POINTER(ctypes.c_float)

#: what the three entry points that do not return a status return
RESTYPES = {
    'remap_arch': ctypes.c_char_p,
    'remap_last_error': ctypes.c_char_p,
    'remap_plan_destroy': None,
}

#: every entry point ``include/remap_hip.h`` declares -> its parameters
PROTOTYPES = {
    'remap_abi_version': (),
    'remap_arch': (),
    'remap_last_error': (),
    'remap_device_count': (),
    'remap_apply_f64': (POINTER(_ApplyArgs), P),
    'remap_csr_from_coo_workspace': (I64, I64, HOST_SIZE),
    'remap_csr_from_coo': (I64, I64, I64, P, P, P, I32, P, P, P, P, P, P,
                           SIZE, P),
    'remap_stream_copy': (P, P, SIZE, P),
    'remap_scan_nan': (P, I32, I64, P, P),
    'remap_scan_nan_kinds': (P, I32, I64, P, P),
    'remap_scan_nan_layout': (P, I32, I64, I64, I64, I64, I64, P, P),
    'remap_groups_workspace': (I64, I64, HOST_SIZE),
    'remap_groups_build': (POINTER(_CSR), P, I32, HOST_I64, I64, I32, I32,
                           P, P, P, P, P, P, P, P, P, SIZE, P),
    'remap_share_build': (POINTER(_CSR), P, I32, P, P, P, P, P, SIZE, P),
    'remap_patches_workspace': (I64, I64, HOST_SIZE),
    'remap_patches_build': (POINTER(_CSR), HOST_I64, I64, I32, I32,
                            P, P, P, P, P, P, P, P, SIZE, P),
    'remap_schedule_sizes': (I64, I64, HOST_SIZE, HOST_SIZE),
    'remap_schedule_auto': (POINTER(_CSR), P, HOST_I64, I32, I64, P, SIZE, P,
                            SIZE, POINTER(_Schedule), P),
    'remap_plan_create': (I64, I64, I64, P, P, P, I32, P, I32, HOST_I64, I32,
                          P, POINTER(P)),
    'remap_plan_destroy': (P,),
    'remap_plan_query': (P, POINTER(_PlanInfo)),
    'remap_plan_apply': (P, POINTER(_Field), P),
    'remap_plan_apply_auto': (P, POINTER(_Field), I64, P, P),
    'remap_pack_columns_workspace': (I64, HOST_SIZE),
    'remap_pack_columns': (P, I64, I64, P, P, P, P, P, SIZE, P),
    'remap_gather_rows': (P, I64, I64, I64, P, I64, I64, P, P),
    'remap_plan_prepare_short_runs': (P, P),
    'remap_clock_probe': (P, I32, P),
    'remap_overlap_latlon_sizes': (POINTER(_OverlapGeom), P, HOST_I64,
                                   HOST_SIZE, P),
    'remap_overlap_latlon': (POINTER(_OverlapGeom), I32, I64, P, SIZE,
                             P, P, P, P, P, P, HOST_I64, P),
    'remap_overlap_meshes_sizes': (POINTER(_OverlapMesh),
                                   POINTER(_OverlapMesh), P, HOST_I64,
                                   HOST_SIZE, P),
    'remap_overlap_meshes': (POINTER(_OverlapMesh), POINTER(_OverlapMesh),
                             I32, I64, P, SIZE, P, P, P, P, P, P, HOST_I64,
                             P),
    'remap_overlap_pieces_sizes': (POINTER(_OverlapPieces),
                                   POINTER(_OverlapPieces), P, HOST_I64,
                                   HOST_SIZE, P),
    'remap_overlap_pieces': (POINTER(_OverlapPieces), POINTER(_OverlapPieces),
                             I32, I64, P, SIZE, P, P, P, P, P, P, HOST_I64,
                             P),
    'remap_overlap_grids_sizes': (POINTER(_OverlapSide),
                                  POINTER(_OverlapSide), HOST_I64, HOST_SIZE,
                                  P),
    'remap_overlap_grids': (POINTER(_OverlapSide), POINTER(_OverlapSide),
                            I32, I64, P, SIZE, P, P, P, P, P, P, HOST_I64, P),
    'remap_nearest_workspace': (I64, I64, HOST_SIZE),
    'remap_nearest': (P, I64, P, I64, P, P, SIZE, P),
    'remap_nearest_k_workspace': (I64, I64, I32, HOST_SIZE),
    'remap_nearest_k': (P, I64, P, I64, I32, P, P, P, SIZE, P),
    'remap_locate_workspace': (I64, I64, I64, HOST_SIZE),
    'remap_locate': (P, I64, P, I64, P, I64, F64, P, P, P, SIZE, P),
    'remap_quads_workspace': (I64, I64, I32, I64, HOST_SIZE),
    'remap_quads': (P, I64, I64, I32, P, I64, F64, P, P, P, SIZE, P),
    'remap_expand_cells': (I64, I32, P, P, P, P, P, P, I32, P, I32,
                           P, P, P, P),
    'remap_cell_areas': (I64, I32, P, P, P, P, P, P),
    'remap_column_fractions_workspace': (I64, HOST_SIZE),
    'remap_column_fractions': (I64, I64, P, I32, P, P, I32, P, P, P, SIZE, P),
    'remap_overlap_moments_workspace': (I64, I32, I64, I32, HOST_SIZE),
    'remap_overlap_moments': (I64, P, P, P, I64, I32, P, P, P, P, P,
                              I64, I32, P, P, P, P, P, P, SIZE, P),
    'remap_gradient_stencils': (I64, I32, P, P, P, P, P, P, P),
    'remap_conserve2nd_sizes': (I64, P, I64, I32, P, P, P, HOST_I64,
                                HOST_SIZE, P),
    'remap_conserve2nd_assemble': (I64, P, P, P, P, I64, I32, P, P, P, P, P,
                                   P, I64, P, I64, P, SIZE, P, P, P, P,
                                   HOST_I64, P),
    'remap_node_rings_workspace': (I64, I64, HOST_SIZE),
    'remap_node_rings': (I64, P, I64, P, P, P, P, SIZE, P),
    'remap_patch_fits': (I64, P, P, P, P, P, P, P),
    'remap_patch_sizes_workspace': (I64, HOST_SIZE),
    'remap_patch_sizes': (I64, P, I64, P, P, P, P, I64, P, P, P, HOST_I64,
                          P, P, SIZE, P),
    'remap_patch_rows': (I64, P, I64, P, P, P, P, P, I64, P, P, P, P, I64,
                         P, P, P, P, P),
    'remap_limit_rows': (POINTER(_LimitArgs), P),
    'remap_apply_sgs': (POINTER(_SgsArgs), P),
    'remap_apply_vector': (POINTER(_VectorArgs), P),
    'remap_apply_levels': (POINTER(_LevelsArgs), P),
    'remap_apply_layers': (POINTER(_LayersArgs), P),
}
# a `_timed` entry is its plain twin with the host `float *` of the phases in
# front of the stream
for _name in ('remap_overlap_pieces', 'remap_nearest', 'remap_locate',
              'remap_quads'):
    PROTOTYPES[_name + '_timed'] = (*PROTOTYPES[_name][:-1], HOST_F32,
                                    PROTOTYPES[_name][-1])
PROTOTYPES['remap_cell_moments'] = PROTOTYPES['remap_cell_areas']

#: every symbol ``include/remap_hip.h`` declares
EXPORTS = tuple(PROTOTYPES)


def declare(lib):
    """Set ``restype`` and ``argtypes`` of every entry point of ``lib``."""
    for name, parameters in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = RESTYPES.get(name, ctypes.c_int)
        fn.argtypes = list(parameters)
