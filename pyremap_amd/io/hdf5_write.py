"""
A small HDF5 writer (numpy only) that produces NetCDF-4 files: the counterpart
of :mod:`pyremap_amd.io.hdf5_lite`, so that a NetCDF-4 input can be answered
with a NetCDF-4 output (what ``ncremap`` does) on images without netCDF4 /
h5py.

Deliberately the oldest, checksum-free flavour of the format (HDF5 File Format
Specification, version-0 superblock): one root group with a symbol table (one
v1 B-tree leaf, one symbol-table node, a local heap), version-1 object
headers, little-endian datasets, version-1 attribute messages, one global
heap collection for the object references of ``DIMENSION_LIST``.

Storage.  A dataset is CONTIGUOUS unless it lies along a record (unlimited)
dimension or is deflated / shuffled; then it is CHUNKED: data layout message
version 3, class 2, the chunks indexed by a version-1 B-tree (node type 1,
real multi-level trees of up to ``2 * CHUNK_BTREE_K`` children per node),
``H5S_UNLIMITED`` maxima in the dataspace on exactly the record axes, a
version-1 filter pipeline message (shuffle, id 2, then deflate, id 1) and the
stored size of every chunk in its B-tree key.  Chunk shapes:
:func:`default_chunks` (one record, split below ``CHUNK_BYTES_MAX``) or the
caller's.  The dimension scale of a record dimension is chunked and unlimited
too -- that is where netCDF-C reads "unlimited" from -- and owns no chunk
when it is a placeholder.  A file without record dimensions and filters is
byte for byte what this writer produced before it knew chunks.

The NetCDF-4 data model on top (as netCDF-C writes it): every dimension is a
dimension-scale dataset (``CLASS = "DIMENSION_SCALE"``, ``NAME``,
``_Netcdf4Dimid``) -- a coordinate variable if one of that name exists, else
an unallocated float dataset named "This is a netCDF dimension but not a
netCDF variable." -- and every variable lists its dimensions in
``DIMENSION_LIST`` (one variable-length list holding one object reference per
axis).  Files are checked against libhdf5 (h5py, ``h5dump``) in
``oracle/check_hdf5_write.py`` and, the chunked ones, in
``tests/check_records_h5py.py``.
"""
import struct
import zlib
from collections import OrderedDict

import numpy as np

from pyremap_amd.io import _parallel

UNDEF = 0xFFFFFFFFFFFFFFFF
_SIG = b'\x89HDF\r\n\x1a\n'
_PURE_DIM = 'This is a netCDF dimension but not a netCDF variable.'

#: Upper bound (exclusive) on the bytes of one chunk under the DEFAULT chunk
#: shape.  The format's own limit is a 32-bit chunk size (< 4 GiB); this one
#: is far lower for two reasons.  A chunk is the unit a reader must fetch --
#: and inflate -- to get at any one value in it, and netCDF-C keeps a chunk
#: only if it fits its per-variable chunk cache, whose default is of this
#: order (16 MiB in recent releases): a larger chunk is inflated again on
#: every partial read.  And it bounds this writer's scratch memory, which is
#: a few chunks (padded copy, shuffled copy, deflated bytes).  One record of a
#: (Time, nCells, nVertLevels) field on a 240 km MPAS mesh still fits whole;
#: finer meshes are split along nCells.  Not a measured optimum.
CHUNK_BYTES_MAX = 16 << 20

#: Chunk B-tree nodes hold up to 2K children.  A version-0 superblock (what
#: this writer emits) has no "indexed storage internal node K" field -- that
#: field arrives with version 1 -- and libhdf5 then assumes its default, 32,
#: when it sizes the nodes it reads: no other value can be written here.
CHUNK_BTREE_K = 32


def _pad8(n):
    return (n + 7) & ~7


# ---------------------------------------------------------------------------
# header messages
# ---------------------------------------------------------------------------

def _datatype(dtype):
    """Datatype message body for a numpy dtype (numbers and S<n> strings)."""
    dt = np.dtype(dtype)
    if dt.kind in 'iu':
        bits = 0x08 if dt.kind == 'i' else 0x00
        return struct.pack('<BBBBI', 0x10, bits, 0, 0, dt.itemsize) + \
            struct.pack('<HH', 0, 8 * dt.itemsize)
    if dt.kind == 'f' and dt.itemsize in (4, 8):
        if dt.itemsize == 4:
            sign, prec, eloc, esize, msize, bias = 31, 32, 23, 8, 23, 127
        else:
            sign, prec, eloc, esize, msize, bias = 63, 64, 52, 11, 52, 1023
        return struct.pack('<BBBBI', 0x11, 0x20, sign, 0, dt.itemsize) + \
            struct.pack('<HHBBBBI', 0, prec, eloc, esize, 0, msize, bias)
    if dt.kind == 'S':
        # fixed length, null terminated, ASCII
        return struct.pack('<BBBBI', 0x13, 0x00, 0, 0, dt.itemsize)
    raise TypeError(f'cannot store dtype {dt} in a NetCDF-4 file')


_REF_TYPE = struct.pack('<BBBBI', 0x17, 0x00, 0, 0, 8)        # object ref
_VLEN_REF_TYPE = struct.pack('<BBBBI', 0x19, 0x00, 0, 0, 16) + _REF_TYPE


def _dataspace(shape, unlimited=()):
    """``unlimited``: one flag per axis (none: no maximum extents stored)."""
    rank = len(shape)
    has_max = bool(rank) and any(unlimited)
    out = struct.pack('<BBB5x', 1, rank, 1 if has_max else 0)
    out += b''.join(struct.pack('<Q', int(n)) for n in shape)
    if has_max:
        out += b''.join(struct.pack('<Q', UNDEF if u else int(n))
                        for n, u in zip(shape, unlimited))
    return out


def _filter_pipeline(shuffle, deflate, itemsize):
    """Filter pipeline message (version 1): shuffle (id 2) before deflate
    (id 1), both optional filters without a name, as libhdf5 writes them."""
    filters = []
    if shuffle:
        filters.append((2, itemsize))
    if deflate:
        filters.append((1, deflate))
    out = struct.pack('<BB6x', 1, len(filters))
    for fid, value in filters:
        # id, name length, flags (optional), one client value + padding
        out += struct.pack('<HHHHI4x', fid, 0, 1, 1, value)
    return out


def default_chunks(shape, unlimited, itemsize):
    """
    The chunk shape of a variable that was given none: 1 along every
    unlimited axis (``unlimited``: one flag per axis), the full extent along
    the others; while that is not under ``CHUNK_BYTES_MAX`` the fixed axes
    are halved (ceiling division) in turn, leading one first.
    """
    chunks = [1 if u else max(int(n), 1) for n, u in zip(shape, unlimited)]
    fixed = [i for i, u in enumerate(unlimited) if not u]
    turn = 0
    while int(np.prod(chunks, dtype=np.int64)) * itemsize >= \
            CHUNK_BYTES_MAX and any(chunks[i] > 1 for i in fixed):
        axis = fixed[turn % len(fixed)]
        turn += 1
        chunks[axis] = -(-chunks[axis] // 2)
    return tuple(chunks)


def _chunk_btree(entries, chunks, address):
    """
    The version-1 B-tree (node type 1) over ``entries`` = ``(stored bytes,
    filter mask, element offsets, address)`` of the chunks in row-major
    order, its nodes laid out from ``address`` on, leaves first: ``(bytes,
    address of the root)``.
    """
    rank = len(chunks)
    key_size = 8 + 8 * (rank + 1)
    node_size = 24 + (2 * CHUNK_BTREE_K + 1) * key_size + \
        2 * CHUNK_BTREE_K * 8

    def key(size, mask, offs):
        return struct.pack(f'<II{rank + 1}Q', size, mask, *offs, 0)

    # the key past the last chunk: beyond it on every axis
    end = key(0, 0, [o + c for o, c in zip(entries[-1][2], chunks)])
    level = [(key(size, mask, offs), addr)
             for size, mask, offs, addr in entries]
    out, depth = [], 0
    while True:
        groups = [level[i:i + 2 * CHUNK_BTREE_K]
                  for i in range(0, len(level), 2 * CHUNK_BTREE_K)]
        addrs = [address + (len(out) + i) * node_size
                 for i in range(len(groups))]
        for i, group in enumerate(groups):
            node = b'TREE' + struct.pack(
                '<BBHQQ', 1, depth, len(group),
                addrs[i - 1] if i else UNDEF,
                addrs[i + 1] if i + 1 < len(groups) else UNDEF)
            node += b''.join(k + struct.pack('<Q', a) for k, a in group)
            node += groups[i + 1][0][0] if i + 1 < len(groups) else end
            out.append(node + b'\x00' * (node_size - len(node)))
        if len(groups) == 1:
            return b''.join(out), addrs[0]
        level = [(group[0][0], a) for group, a in zip(groups, addrs)]
        depth += 1


def _message(mtype, body, flags=0):
    body = body + b'\x00' * (_pad8(len(body)) - len(body))
    if len(body) > 0xFFF8:
        raise ValueError('a header message exceeds 64 KiB (attribute too '
                         'long for this writer)')
    return struct.pack('<HHB3x', mtype, len(body), flags) + body


def _attribute(name, dtype_body, space_body, data):
    nm = name.encode('utf-8') + b'\x00'
    body = struct.pack('<BxHHH', 1, len(nm), len(dtype_body),
                       len(space_body))
    for part in (nm, dtype_body, space_body):
        body += part + b'\x00' * (_pad8(len(part)) - len(part))
    return _message(0x0C, body + data)


def _attr_value(name, value):
    """An attribute message for a python / numpy value."""
    if isinstance(value, bytes):
        value = value.decode('utf-8', 'replace')
    if isinstance(value, str):
        raw = value.encode('utf-8') + b'\x00'
        return _attribute(name, _datatype(f'S{len(raw)}'), _dataspace(()),
                          raw)
    arr = np.asarray(value)
    if arr.dtype.kind in 'US':
        return _attr_value(name, ' '.join(str(v) for v in arr.reshape(-1)))
    if arr.dtype.kind == 'b':
        arr = arr.astype(np.int8)
    if arr.dtype.kind not in 'iuf':
        return _attr_value(name, str(value))
    arr = np.ascontiguousarray(arr.astype(arr.dtype.newbyteorder('<')))
    # numbers are 1-D arrays in netCDF (even single ones)
    return _attribute(name, _datatype(arr.dtype),
                      _dataspace((arr.size,)), arr.tobytes())


def _object_header(messages):
    body = b''.join(messages)
    return struct.pack('<BxHII4x', 1, len(messages), 1, len(body)) + body


# ---------------------------------------------------------------------------
# the file
# ---------------------------------------------------------------------------

class _Dataset:
    def __init__(self, name, data, dims, attrs, allocate=True):
        self.name = name
        self.data = data
        self.dims = tuple(dims)
        self.attrs = attrs
        self.allocate = allocate
        self.header_addr = None
        self.data_addr = None
        self.ref_slots = []       # global-heap object indices, one per axis
        self.chunks = None        # chunk shape; None: contiguous storage
        self.unlimited = ()       # one flag per axis (chunked datasets)
        self.deflate = 0          # zlib level, 0: no deflate filter
        self.shuffle = False
        self.btree_addr = None    # chunk B-tree (None: no chunk written)


def _is_deferred(data):
    return hasattr(data, 'load') and not isinstance(data, np.ndarray)


def _write_chunks(f, ds, data, fill, tail):
    """
    The chunks of ``data`` from file position ``tail`` on, each NaN ->
    ``fill`` substituted, shuffled and deflated as ``ds`` asks, then the
    B-tree that indexes them; sets ``ds.btree_addr`` and returns the new end
    of the file.  One chunk is in flight at a time.
    """
    shape, chunks = data.shape, ds.chunks
    item = data.dtype.itemsize
    plain = not (ds.deflate or ds.shuffle)
    grid = [-(-s // c) for s, c in zip(shape, chunks)]
    entries = []
    for index in np.ndindex(*grid):
        offs = tuple(i * c for i, c in zip(index, chunks))
        block = data[tuple(slice(o, o + c) for o, c in zip(offs, chunks))]
        if block.shape != chunks:
            # a ragged edge: chunks are stored whole
            full = np.zeros(chunks, dtype=data.dtype)
            full[tuple(slice(0, n) for n in block.shape)] = block
            block = full
        f.seek(tail)
        if plain and block.flags['C_CONTIGUOUS'] and \
                block.dtype.kind in 'iuf':
            # the array's own memory goes to the file
            size = _parallel.write_at(f, block, nan_fill=fill)
        else:
            if fill is not None:
                block = np.array(block, copy=True, order='C')
                block[np.isnan(block)] = fill
            raw = np.ascontiguousarray(block).reshape(-1).view(np.uint8)
            if ds.shuffle and item > 1:
                raw = np.ascontiguousarray(raw.reshape(-1, item).T)
            blob = zlib.compress(raw, ds.deflate) if ds.deflate else \
                raw.tobytes()
            del raw, block
            size = len(blob)
            f.write(blob)
            del blob
        entries.append((size, 0, offs, tail))
        tail += _pad8(size)
    if entries:
        tree, ds.btree_addr = _chunk_btree(entries, chunks, tail)
        f.seek(tail)
        f.write(tree)
        tail += len(tree)
    return tail


def write_netcdf4(filename, dimensions, variables, attrs=None,
                  unlimited=(), nan_fill=None, auto_fill=None,
                  encoding=None):
    """
    ``auto_fill``: variable name -> fill value for variables whose data is
    PRODUCED ON DEMAND (an object with ``shape``, ``dtype``, ``load()`` and
    optionally ``prefetch()``): each is loaded when the writer reaches it,
    written and dropped (the next one started meanwhile), and gets that
    value as ``_FillValue`` -- and in place of its NaNs -- iff its values
    hold NaNs.  Their object headers are laid out with the attribute and
    written last; where it turns out not to be needed a NIL message of the
    same size takes its place.


    ``dimensions``: ordered name -> length; ``variables``: iterable of
    ``(name, dims, ndarray, attrs)``; ``attrs``: global attributes;
    ``nan_fill``: variable name -> value stored in place of its NaNs
    (substituted chunk by chunk while writing);
    ``unlimited``: names of the record dimensions.  Every variable along one
    -- and its dimension scale, placeholders included -- is stored CHUNKED
    with an unlimited maximum extent on those axes (HDF5 allows such maxima
    on chunked datasets only); a record dimension may have length 0;
    ``encoding``: variable name -> ``{'zlib': bool, 'complevel': 0-9 (4),
    'shuffle': bool, 'chunksizes': shape}``, xarray's keys.  A deflated or
    shuffled variable is chunked too, whatever its dimensions (scalars are
    never filtered); NaNs are replaced before the filters run.  A chunk
    shape given here is used as given, any other is
    :func:`default_chunks`.  With neither the file is, byte for byte, the
    contiguous one this writer has always produced.

    Layout: object headers and contiguous data first, at addresses known
    before anything is written; then, variable by variable, the chunks of
    each chunked dataset followed by its B-tree (a deflated chunk's size is
    known only once it exists, for on-demand variables not even the values
    are), and last its object header with the tree's address -- a field of
    fixed size -- and the superblock with the end of the file.
    """
    attrs = OrderedDict(attrs or {})
    encoding = {k: dict(v or {}) for k, v in (encoding or {}).items()}
    unlimited = set(unlimited or ())
    auto_fill = dict(auto_fill or {})
    nan_fill = dict(nan_fill or {})
    dimensions = OrderedDict((k, int(v)) for k, v in dimensions.items())
    datasets = OrderedDict()
    for name, dims, data, vattrs in variables:
        if _is_deferred(data):
            if tuple(data.shape) != tuple(dimensions[d] for d in dims):
                raise ValueError(f'{name}: shape {data.shape} does not '
                                 f'match dimensions {dims}')
            datasets[name] = _Dataset(name, data, dims,
                                      OrderedDict(vattrs or {}))
            continue
        arr = np.asarray(data)
        if arr.dtype.kind == 'U':
            arr = np.char.encode(arr, 'utf-8')
        if arr.dtype.kind == 'b':
            arr = arr.astype(np.int8)
        if arr.dtype.kind in 'iuf':
            # (no copy when the data is little-endian already: a remapped
            # field is as large as memory allows)
            arr = arr.astype(arr.dtype.newbyteorder('<'), copy=False)
        if tuple(arr.shape) != tuple(dimensions[d] for d in dims):
            raise ValueError(f'{name}: shape {arr.shape} does not match '
                             f'dimensions {dims}')
        if arr.ndim:                 # (ascontiguousarray makes 0-d 1-d)
            arr = np.ascontiguousarray(arr)
        datasets[name] = _Dataset(name, arr, dims, OrderedDict(vattrs or {}))
    # dimension scales: coordinate variables, or placeholders
    dim_ids = {d: i for i, d in enumerate(dimensions)}
    for d, n in dimensions.items():
        ds = datasets.get(d)
        if ds is None or ds.dims != (d,):
            if ds is not None:
                raise ValueError(
                    f'variable {d} shares its name with a dimension but is '
                    f'not 1-D along it: NetCDF-4 files written here cannot '
                    f'hold that')
            datasets[d] = _Dataset(d, np.zeros(n, dtype='<f4'), (d,),
                                   OrderedDict(), allocate=False)
    names = sorted(datasets, key=lambda s: s.encode('utf-8'))
    unknown = sorted(set(encoding) - set(datasets))
    if unknown:
        raise ValueError(f'encoding given for {unknown}: no such variables')
    for ds in datasets.values():
        enc = encoding.get(ds.name, {})
        extra = sorted(set(enc) - {'zlib', 'complevel', 'shuffle',
                                   'chunksizes'})
        if extra:
            raise ValueError(f'{ds.name}: unknown encoding keys {extra}')
        shape = tuple(ds.data.shape)
        if not shape:
            continue                          # scalars: contiguous, always
        item = np.dtype(ds.data.dtype).itemsize
        ds.unlimited = tuple(d in unlimited for d in ds.dims)
        ds.deflate = int(enc.get('complevel', 4)) if enc.get('zlib') else 0
        if not 0 <= ds.deflate <= 9:
            raise ValueError(f'{ds.name}: complevel {ds.deflate} is not a '
                             f'zlib level (0-9)')
        ds.shuffle = bool(enc.get('shuffle', False))
        given = enc.get('chunksizes')
        if given is not None:
            ds.chunks = tuple(int(c) for c in given)
            # (HDF5 lets a chunk exceed the extent of an unlimited axis
            # only)
            if len(ds.chunks) != len(shape) or min(ds.chunks) < 1 or any(
                    c > max(n, 1) and not u for c, n, u in
                    zip(ds.chunks, shape, ds.unlimited)):
                raise ValueError(f'{ds.name}: chunksizes {given} do not '
                                 f'fit shape {shape}')
        elif any(ds.unlimited) or ds.deflate or ds.shuffle:
            ds.chunks = default_chunks(shape, ds.unlimited, item)
        if ds.chunks is not None and \
                int(np.prod(ds.chunks, dtype=object)) * item >= 1 << 32:
            raise ValueError(f'{ds.name}: a chunk of shape {ds.chunks} '
                             f'exceeds the 32-bit chunk size of HDF5')

    # -- global heap: one 8-byte object per (variable, axis) reference -------
    heap_objects = []          # dimension name of each object, index = i + 1
    for name in names:
        ds = datasets[name]
        if name in dimensions and ds.dims == (name,):
            continue                      # a scale does not list itself
        for d in ds.dims:
            heap_objects.append(d)
            ds.ref_slots.append(len(heap_objects))

    def dataset_messages(ds, gheap_addr, reserve=False):
        dtype = np.dtype(ds.data.dtype).newbyteorder('<')
        msgs = [_message(0x01, _dataspace(ds.data.shape, ds.unlimited
                                          if ds.chunks is not None else ())),
                _message(0x03, _datatype(dtype), flags=0x01)]
        if ds.chunks is None:
            nbytes = ds.data.nbytes
            addr = (ds.data_addr or 0) if (ds.allocate and nbytes) else UNDEF
            msgs.append(_message(0x08, struct.pack('<BBQQ', 3, 1, addr,
                                                   nbytes)))
        else:
            # chunked (layout version 3, class 2): the B-tree's address, then
            # the chunk shape with the element size as one more dimension
            if ds.deflate or ds.shuffle:
                msgs.append(_message(0x0B, _filter_pipeline(
                    ds.shuffle, ds.deflate, dtype.itemsize)))
            msgs.append(_message(0x08, struct.pack(
                f'<BBBQ{len(ds.chunks) + 1}I', 3, 2, len(ds.chunks) + 1,
                UNDEF if ds.btree_addr is None else ds.btree_addr,
                *ds.chunks, dtype.itemsize)))
        if ds.name in dimensions and ds.dims == (ds.name,):
            label = ds.name if ds.allocate else \
                f'{_PURE_DIM}{dimensions[ds.name]:10d}'
            msgs.append(_attr_value('CLASS', 'DIMENSION_SCALE'))
            msgs.append(_attr_value('NAME', label))
            msgs.append(_attribute('_Netcdf4Dimid', _datatype('<i4'),
                                   _dataspace(()),
                                   struct.pack('<i', dim_ids[ds.name])))
        elif ds.ref_slots:
            data = b''.join(struct.pack('<IQI', 1, gheap_addr, slot)
                            for slot in ds.ref_slots)
            msgs.append(_attribute('DIMENSION_LIST', _VLEN_REF_TYPE,
                                   _dataspace((len(ds.ref_slots),)), data))
        for key, value in ds.attrs.items():
            msgs.append(_attr_value(key, value))
        if _is_deferred(ds.data) and ds.name in auto_fill:
            # the _FillValue of a variable whose values are not known yet:
            # reserved in the layout, written iff NaNs turned up, a NIL
            # message of the same size otherwise
            fill = _attr_value('_FillValue', auto_fill[ds.name])
            if reserve or ds.name in nan_fill:
                msgs.append(fill)
            else:
                msgs.append(_message(0x00, b'\x00' * (len(fill) - 8)))
        return msgs

    # -- pass 1: sizes (addresses do not change any size) --------------------
    leaf_k = max(4, (len(names) + 1) // 2)
    internal_k = 16
    root_msgs = [_message(0x11, struct.pack('<QQ', 0, 0))] + \
        [_attr_value(k, v) for k, v in attrs.items()]
    root_header = _object_header(root_msgs)
    btree_size = 24 + 2 * internal_k * 8 + (2 * internal_k + 1) * 8
    heap_names = [b'']
    heap_names += [n.encode('utf-8') for n in names]
    name_offsets, off = [], 0
    for nm in heap_names:
        name_offsets.append(off)
        off += _pad8(len(nm) + 1)
    heap_data_size = off + 16                    # + one free block
    snod_size = 8 + 2 * leaf_k * 40
    gheap_used = 16 + len(heap_objects) * (16 + 8)
    gheap_size = max(4096, _pad8(gheap_used + 16))

    pos = 96                                     # superblock
    root_addr = pos
    pos += _pad8(len(root_header))
    btree_addr = pos
    pos += btree_size
    heap_addr = pos
    pos += 32
    heap_data_addr = pos
    pos += heap_data_size
    snod_addr = pos
    pos += snod_size
    gheap_addr = pos
    pos += gheap_size
    for name in names:
        ds = datasets[name]
        ds.header_addr = pos
        pos += _pad8(len(_object_header(dataset_messages(ds, gheap_addr,
                                                         reserve=True))))
    for name in names:
        ds = datasets[name]
        if ds.chunks is None and ds.allocate and ds.data.nbytes:
            ds.data_addr = pos
            pos += _pad8(ds.data.nbytes)
    eof = pos                 # (chunked datasets are appended from here on)

    # -- pass 2: bytes -------------------------------------------------------
    with open(filename, 'wb') as f:
        def put(addr, blob, fill=None):
            f.seek(addr)
            if isinstance(blob, np.ndarray):
                # large arrays: several cores
                _parallel.write_at(f, blob, nan_fill=fill)
            else:
                f.write(blob)

        root_msgs[0] = _message(0x11, struct.pack('<QQ', btree_addr,
                                                  heap_addr))
        put(root_addr, _object_header(root_msgs))
        # B-tree: one leaf entry -> the symbol-table node
        bt = b'TREE' + struct.pack('<BBHQQ', 0, 0, 1, UNDEF, UNDEF)
        bt += struct.pack('<QQQ', 0, snod_addr, name_offsets[-1])
        put(btree_addr, bt + b'\x00' * (btree_size - len(bt)))
        # local heap: names, then one free block to the end
        put(heap_addr, b'HEAP' + struct.pack('<B3xQQQ', 0, heap_data_size,
                                             heap_data_size - 16,
                                             heap_data_addr))
        seg = bytearray(heap_data_size)
        for nm, o in zip(heap_names, name_offsets):
            seg[o:o + len(nm)] = nm
        seg[heap_data_size - 16:] = struct.pack('<QQ', 1, 16)
        put(heap_data_addr, bytes(seg))
        # symbol-table node, entries sorted by name
        sn = b'SNOD' + struct.pack('<BxH', 1, len(names))
        for name, o in zip(names, name_offsets[1:]):
            sn += struct.pack('<QQII16x', o, datasets[name].header_addr, 0,
                              0)
        put(snod_addr, sn + b'\x00' * (snod_size - len(sn)))
        # global heap collection: the object references
        gh = b'GCOL' + struct.pack('<B3xQ', 1, gheap_size)
        for i, d in enumerate(heap_objects):
            gh += struct.pack('<HH4xQQ', i + 1, 1, 8,
                              datasets[d].header_addr)
        free = gheap_size - len(gh)
        gh += struct.pack('<HH4xQ', 0, 0, free)
        put(gheap_addr, gh + b'\x00' * (gheap_size - len(gh)))
        deferred = [n for n in names if _is_deferred(datasets[n].data)]
        for name in names:
            ds = datasets[name]
            data = ds.data
            if _is_deferred(data):
                later = deferred[deferred.index(name) + 1:]
                if later and hasattr(datasets[later[0]].data, 'prefetch'):
                    datasets[later[0]].data.prefetch()
                arr = np.asarray(data.load())
                if tuple(arr.shape) != tuple(data.shape) or \
                        arr.dtype.itemsize != np.dtype(data.dtype).itemsize:
                    raise ValueError(
                        f'{name}: produced {arr.dtype} {arr.shape}, '
                        f'announced {data.dtype} {tuple(data.shape)}')
                arr = np.ascontiguousarray(
                    arr.astype(arr.dtype.newbyteorder('<'), copy=False))
                if name in auto_fill and _parallel.any_nan(arr):
                    nan_fill[name] = auto_fill[name]
                data = arr
            if ds.chunks is not None:
                if ds.allocate:
                    eof = _write_chunks(f, ds, data, nan_fill.get(name), eof)
            elif ds.data_addr is not None:
                # the array's own memory goes to the file (no tobytes copy)
                put(ds.data_addr, data
                    if data.dtype.kind in 'iuf' and data.size
                    else data.tobytes(), nan_fill.get(name))
            del data
            # (after the data: a deferred variable's _FillValue is known now)
            put(ds.header_addr,
                _object_header(dataset_messages(ds, gheap_addr)))
        # (last: the end of the file moves with every chunked dataset)
        sb = _SIG + struct.pack('<BBBBBBBB', 0, 0, 0, 0, 0, 8, 8, 0)
        sb += struct.pack('<HHI', leaf_k, internal_k, 0)
        sb += struct.pack('<QQQQ', 0, UNDEF, eof, UNDEF)
        sb += struct.pack('<QQII', 0, root_addr, 1, 0)
        sb += struct.pack('<QQ', btree_addr, heap_addr)
        put(0, sb)
        f.truncate(eof)
