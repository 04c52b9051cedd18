"""
Host-resident fields through the engine: numpy in -> numpy out, as
``Remapper.remap_numpy(ds)`` hands them over (the reference materialises the
whole ``(n_a, K)`` field in RAM, ``remap_numpy.py:254-256``, and runs scipy on
it; here the field crosses PCIe once each way around one fused launch).

What this module is about is everything AROUND the 0.4 ms kernel:

* results land in PINNED host memory taken from (and, when the caller drops
  the array, returned to) torch's caching host allocator -- the first touch
  of a fresh 1 GB pageable result cost ~110 ms, five times the transfer;
* no host synchronisation between upload and launch: the reference's
  ``isnan(values).any()`` test (``remap_numpy.py:201-204``) runs on the
  device (``remap_scan_nan``) and the two candidate launches are gated on
  its flag (``remap_apply_args.gate``);
* upload, kernel and download of successive batches overlap on three
  streams when the field has leading batch dims and the mode is known
  (PCIe is full duplex);
* nothing blocks until the caller asks for the data: a Dataset's variables
  are all enqueued before the first result is awaited.
"""
import ctypes
import os
import queue
import threading
import weakref

import numpy as np

from pyremap_amd import engine

#: target bytes per pipelined chunk (large enough for full PCIe rate, small
#: enough that the first download starts early)
CHUNK_BYTES = 64 << 20

#: Results are handed out in PINNED host memory (page-locked: a resource the
#: OS does not swap).  At most this many bytes of results may be alive at a
#: time in pinned memory; beyond it a result lands in ordinary pageable
#: memory (slower: first-touch page faults) rather than pinning without
#: bound.  Environment: PYREMAP_AMD_PINNED_LIMIT (bytes).
def _default_pinned_limit():
    """min(4 GiB, a quarter of the machine's RAM): freed result blocks go
    back to torch's caching HOST allocator, which keeps them pinned, so the
    budget is what a long-lived process may end up holding page-locked."""
    try:
        ram = os.sysconf('SC_PAGE_SIZE') * os.sysconf('SC_PHYS_PAGES')
    except (ValueError, OSError, AttributeError):
        ram = 16 << 30
    return min(4 << 30, ram // 4)


PINNED_LIMIT = int(os.environ.get('PYREMAP_AMD_PINNED_LIMIT',
                                  _default_pinned_limit()))

#: device buffers of the batch pipeline: this many chunk-sized slots each
#: for the source and the result (bounded device memory whatever the field)
RING_SLOTS = 4

#: helper threads feeding pageable uploads (one stream each).  More than
#: one does not help: two feeders on two streams were measured SLOWER (0.96 GB
#: + 1.06 GB: 31-41 ms against 23.6; a 7.7 GB series 444-473 ms against
#: 326-342) -- the runtime's pageable-copy staging is shared.
N_UPLOADERS = 1

#: the column-panel pipeline of (n_a, K) host arrays: columns per panel (1
#: KiB rows of float64: hipMemcpy2DAsync moves such panels at the rate of a
#: contiguous copy, 53-57 GB/s either way, tools/pcie_panel_probe.py) and the
#: fewest panels worth the extra launches
PANEL_COLUMNS = 128
PANEL_MIN = 3

#: the handle of :func:`_hip`: ``None`` = not looked for yet, ``False`` = no
#: runtime could be loaded
_hip_runtime = [None]

#: sonames tried after torch's own copy: the name a process that runs torch
#: has already loaded, then the versioned ones of a system ROCm
_HIP_SONAMES = ('libamdhip64.so', 'libamdhip64.so.7', 'libamdhip64.so.6',
                'libamdhip64.so.5')


def _hip():
    """The HIP runtime torch itself uses (2-D copies: torch's strided
    ``copy_`` between host and device goes through a host-side contiguous
    copy at 4-5 GB/s), resolved once: torch's lib directory (the wheels
    carry their own), then the sonames of a system ROCm that torch was built
    against.  ``None`` when none of them loads -- the column-panel route
    then declines and the plain form answers."""
    if _hip_runtime[0] is None:
        torch = engine._torch()
        names = (os.path.join(os.path.dirname(torch.__file__), 'lib',
                              'libamdhip64.so'),) + _HIP_SONAMES
        _hip_runtime[0] = False
        for name in names:
            try:
                lib = ctypes.CDLL(name)
                lib.hipMemcpy2DAsync.restype = ctypes.c_int
            except (OSError, AttributeError):
                continue
            lib.hipMemcpy2DAsync.argtypes = [
                ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                ctypes.c_int, ctypes.c_void_p]
            _hip_runtime[0] = lib
            break
        else:
            _log_once('hip', 'no HIP runtime could be loaded for 2-D '
                      'copies; (n_a, K) host arrays take the plain form')
    return _hip_runtime[0] or None


def _copy_2d(dst_ptr, dst_pitch, src_ptr, src_pitch, width, height, kind,
             stream):
    rc = _hip().hipMemcpy2DAsync(dst_ptr, dst_pitch, src_ptr, src_pitch,
                                 width, height, kind,
                                 ctypes.c_void_p(stream.cuda_stream))
    if rc != 0:
        raise engine.EngineError(f'hipMemcpy2DAsync failed ({rc})')


_streams = {}
_extra_streams = {}
_pinned_alive = [0]
_pinned_lock = threading.Lock()


_logged = set()


def _log_once(key, message):
    if key not in _logged:
        _logged.add(key)
        import logging
        logging.getLogger('pyremap_amd').info(message)


def _host_buffer(shape, dtype):
    """A result buffer: pinned while the budget lasts, pageable beyond."""
    torch = engine._torch()
    nbytes = _prod(shape) * torch.empty((), dtype=dtype).element_size()
    with _pinned_lock:
        pin = _pinned_alive[0] + nbytes <= PINNED_LIMIT
        if pin:
            _pinned_alive[0] += nbytes
    if pin:
        try:
            return torch.empty(shape, dtype=dtype, pin_memory=True), nbytes
        except RuntimeError:
            # page-locking refused (ulimit -l, little RAM): hand the cached
            # pinned blocks back and degrade to pageable memory
            _release_pinned(nbytes)
            try:
                torch._C._host_emptyCache()
            except AttributeError:
                pass
            _log_once('pin', 'pinned host memory refused; results land in '
                      'pageable memory')
    return torch.empty(shape, dtype=dtype), 0


def _release_pinned(nbytes):
    with _pinned_lock:
        _pinned_alive[0] -= nbytes


def pinned_bytes_alive():
    """Bytes of results currently alive in pinned host memory."""
    return _pinned_alive[0]


def _side_streams(device):
    torch = engine._torch()
    key = (device.type, device.index)
    if key not in _streams:
        _streams[key] = (torch.cuda.Stream(device=device),
                         torch.cuda.Stream(device=device))
    return _streams[key]


#: a field (source + result) larger than this fraction of the free device
#: memory is not made resident whole to decide the masked/unmasked branch
DEVICE_FRACTION = 0.5


def _sampled_nan(values, samples=1 << 16):
    """Is there a NaN among ~``samples`` evenly strided elements?"""
    flat = values.reshape(-1)
    step = max(1, flat.size // samples)
    return bool(np.isnan(flat[::step]).any())


def _any_nan(values, chunk=CHUNK_BYTES):
    """``np.isnan(values).any()`` with an early exit, chunk by chunk."""
    flat = values.reshape(-1)
    step = max(1, chunk // values.dtype.itemsize)
    for i in range(0, flat.size, step):
        if np.isnan(flat[i:i + step]).any():
            return True
    return False


def _extra_stream(device, k):
    torch = engine._torch()
    key = (device.type, device.index, k)
    if key not in _extra_streams:
        _extra_streams[key] = torch.cuda.Stream(device=device)
    return _extra_streams[key]


def _prod(seq):
    out = 1
    for s in seq:
        out *= int(s)
    return out


def _as_uploadable(values):
    values = np.asarray(values)
    if values.dtype.kind not in 'fiub':
        raise TypeError(f'cannot remap an array of dtype {values.dtype}')
    if values.dtype not in (np.float64, np.float32):
        # scipy upcasts everything else to float64 before the product
        values = values.astype(np.float64)
    if not values.flags['C_CONTIGUOUS'] or not values.flags['WRITEABLE']:
        values = np.array(values, order='C')
    return values


class Pending:
    """
    A remap whose transfers and launch are enqueued.  :meth:`result` waits
    for the download and returns ``data`` (NaN where the reference masks) or
    ``(data, mask)``; the arrays live in pinned host memory that returns to
    torch's pool when they are garbage collected.
    """

    def __init__(self, event, out, mask, pinned=(0, 0), recheck=None):
        self._event = event
        self._out = out
        self._mask = mask
        self._pinned = list(pinned)    # pinned bytes of (out, mask)
        self._done = None
        # the column-panel pipeline's second look (mode 'auto' taken as
        # frac_b panel by panel: a NaN found by the device scans means the
        # whole field over again in the masked mode); called once the
        # downloads are in
        self._recheck = recheck
        # a Pending dropped without result() gives its budget back
        self._guard = weakref.finalize(self, _release_pinned, sum(pinned))

    def result(self):
        if self._done is not None:
            return self._done
        if self._event is not None:
            self._event.synchronize()
            self._event = None
        if self._recheck is not None:
            recheck, self._recheck = self._recheck, None
            recheck()
        # the budget now follows the ARRAYS (views keep their base alive)
        self._guard.detach()
        data = self._out.numpy()
        weakref.finalize(data, _release_pinned, self._pinned[0])
        if self._mask is None:
            self._done = data
            return data
        mask = self._mask.numpy()
        weakref.finalize(mask, _release_pinned, self._pinned[1])
        self._done = (data, mask.view(np.bool_))
        return self._done


class OnDevice:
    """
    A remap whose result STAYS ON THE DEVICE until asked for
    (``remap_host_array(..., keep_on_device=True)``): :meth:`result`
    allocates the (pinned) host buffer, downloads and returns the data.  The
    streaming file path starts the next variable this way while the current
    one is being written: the host holds one result and, briefly, one input
    -- HBM holds what is in flight (288 GB of it).
    """

    def __init__(self, y_d, out_shape):
        torch = engine._torch()
        self._y_d = y_d
        self._out_shape = out_shape
        self._done = None
        # the launch that produces y_d sits on the stream that is current
        # NOW; result() may be called under another one
        self._ready = torch.cuda.Event()
        self._ready.record(torch.cuda.current_stream(y_d.device))

    def result(self):
        if self._done is not None:
            return self._done
        torch = engine._torch()
        y_d, self._y_d = self._y_d, None
        with torch.cuda.device(y_d.device):
            out_h, pinned = _host_buffer(self._out_shape, torch.float64)
            try:
                stream = torch.cuda.current_stream(y_d.device)
                stream.wait_event(self._ready)
                out_h.copy_(y_d, non_blocking=True)
                y_d.record_stream(stream)
                stream.synchronize()
            except BaseException:
                _release_pinned(pinned)
                raise
        data = out_h.numpy()
        weakref.finalize(data, _release_pinned, pinned)
        self._done = data
        return data


#: a Dataset's variables of one shape and dtype, each at most this large,
#: travel and are remapped TOGETHER (remap_host_batch), at most
#: BATCH_TOTAL_BYTES of them at a time
BATCH_VAR_BYTES = 16 << 20
BATCH_TOTAL_BYTES = 256 << 20


class PendingBatch:
    """Several same-shaped arrays remapped as ONE stacked array
    (:func:`remap_host_batch`): :meth:`result` waits for the one download and
    returns the list of result arrays -- views of one pinned buffer, which
    returns to torch's pool when the last of them is collected."""

    def __init__(self, event, out, pinned):
        self._event, self._out, self._pinned = event, out, pinned
        self._done = None
        self._guard = weakref.finalize(self, _release_pinned, pinned)

    def result(self):
        if self._done is None:
            self._event.synchronize()
            self._guard.detach()
            whole = self._out.numpy()
            weakref.finalize(whole, _release_pinned, self._pinned)
            self._done = [whole[v] for v in range(whole.shape[0])]
            self._out = None
        return self._done


def remap_host_batch(plan, dst_grid_dims, arrays, remap_axes, *, mode,
                     threshold=None, flags=0):
    """
    ``[remap_host_array(a, ...).result() for a in arrays]`` for host arrays
    of ONE shape and dtype -- the dozens of ``(Time = 1, nCells)`` variables
    of a climatology Dataset, each a few microseconds of device work behind
    ~150 us of per-call host work (reference: the per-variable loop of
    ``remap_numpy.py:42-55``) -- as one stacked array: V uploads into one
    device buffer, the reference's per-variable ``isnan(values).any()``
    (``:201-204``) as one device reduction and ONE read-back of V flags, one
    launch per run of variables that take the same branch, one download.
    The values of every variable are those of its own call, bit for bit:
    a variable is a set of whole batches of the stacked launch, and every
    kernel family sums a row's entries in the same order.
    ``mode``: ``'fracb'`` or ``'auto'``.  Returns a :class:`PendingBatch`.
    """
    torch = engine.require_gpu()
    device = plan.device
    arrays = [_as_uploadable(a) for a in arrays]
    shape, dtype = arrays[0].shape, arrays[0].dtype
    if any(a.shape != shape or a.dtype != dtype for a in arrays):
        raise ValueError('remap_host_batch: arrays of one shape and dtype')
    if mode not in ('fracb', 'auto'):
        raise ValueError(f'unknown mode {mode!r}')
    if mode == 'auto' and threshold is None:
        raise ValueError('the masked branch needs a threshold')
    V, nd = len(arrays), len(shape)
    axes, dst_shape = engine.check_field_extents(
        plan.n_a, plan.n_b, plan.n_b_global, dst_grid_dims, shape,
        remap_axes)
    lead = min(axes)
    out_shape = [V] + list(shape[:lead]) + dst_shape + \
        [int(shape[ax]) for ax in range(lead, nd) if ax not in axes]
    stacked_axes = [a + 1 for a in axes]
    # sub-batches on three streams: the variables of sub-batch s + 1 travel
    # up while those of s are computed and travel down (PCIe is full duplex)
    n_sub = 1 if V < 8 else min(4, V // 4)
    bounds = [V * k // n_sub for k in range(n_sub + 1)]
    up, down = _side_streams(device)
    with torch.cuda.device(device):
        main = torch.cuda.current_stream(device)
        x_d = torch.empty((V,) + tuple(shape), device=device,
                          dtype=torch.from_numpy(arrays[0][:0]).dtype)
        y_d = torch.empty(out_shape, dtype=torch.float64, device=device)
        out_h, pinned = _host_buffer(out_shape, torch.float64)
        try:
            up.wait_stream(main)
            down.wait_stream(main)
            # a copy from pageable memory holds its host thread until it is
            # staged (1.9 MB: ~40 us): a feeder thread issues the uploads,
            # this one the launches and downloads of what has arrived
            arrivals = queue.Queue()

            def uploader():
                try:
                    with torch.cuda.device(device), torch.cuda.stream(up):
                        for k in range(n_sub):
                            for v in range(bounds[k], bounds[k + 1]):
                                x_d[v].copy_(torch.from_numpy(arrays[v]),
                                             non_blocking=True)
                            ev = torch.cuda.Event()
                            ev.record(up)
                            arrivals.put(ev)
                except BaseException as exc:   # noqa: BLE001 - handed over
                    arrivals.put(exc)

            feeder = threading.Thread(target=uploader, daemon=True,
                                      name='pyremap_amd.batch_uploader')
            feeder.start()
            for k in range(n_sub):
                lo, hi = bounds[k], bounds[k + 1]
                uploaded = arrivals.get()
                if isinstance(uploaded, BaseException):
                    feeder.join()
                    raise uploaded
                main.wait_event(uploaded)
                if mode == 'fracb':
                    engine.remap_tensor(plan, dst_grid_dims, x_d[lo:hi],
                                        stacked_axes, engine.MODE_FRACB,
                                        flags=flags, out=y_d[lo:hi])
                else:
                    # which variables hold a NaN: one reduction, one
                    # read-back (it waits for this sub-batch's uploads --
                    # they are needed anyway)
                    has = torch.isnan(x_d[lo:hi].view(hi - lo, -1)).any(
                        dim=1).cpu().tolist()
                    v0 = 0
                    while v0 < hi - lo:
                        v1 = v0 + 1
                        while v1 < hi - lo and has[v1] == has[v0]:
                            v1 += 1
                        engine.remap_tensor(
                            plan, dst_grid_dims, x_d[lo + v0:lo + v1],
                            stacked_axes,
                            engine.MODE_MASKED if has[v0] else
                            engine.MODE_FRACB,
                            threshold=float(threshold) if has[v0] else 0.0,
                            flags=flags, out=y_d[lo + v0:lo + v1])
                        v0 = v1
                ev = torch.cuda.Event()
                ev.record(main)
                down.wait_event(ev)
                with torch.cuda.stream(down):
                    out_h[lo:hi].copy_(y_d[lo:hi], non_blocking=True)
            feeder.join()
            x_d.record_stream(up)
            y_d.record_stream(down)
            event = torch.cuda.Event()
            event.record(down)
            # (the caller's stream sees the batch finished as well)
            main.wait_event(event)
        except BaseException:
            # The feeder may still be copying from `arrays` into x_d on the
            # upload stream, downloads of earlier sub-batches may still be
            # writing out_h: wait for all of it BEFORE the buffers go back
            # to their allocators -- a block handed out again while a side
            # stream still writes into it is silent corruption.  (The feeder
            # ends by itself: its list is finite.)
            try:
                feeder.join()
            except NameError:
                pass
            up.synchronize()
            down.synchronize()
            _release_pinned(pinned)
            raise
    return PendingBatch(event, out_h, pinned)


def remap_host_array(plan, dst_grid_dims, values, remap_axes, *, mode,
                     threshold=None, want_mask=False, flags=0,
                     host_mask=None, keep_on_device=False, limiter=None,
                     row_weight=None):
    """
    Enqueue the remap of one host array and return a :class:`Pending`
    (``keep_on_device``: an :class:`OnDevice` -- upload and launch are
    enqueued, the download waits for ``result()``).

    ``mode``: ``'fracb'`` (unmasked branch), ``'masked'`` (NaN-as-mask with
    renormalisation; ``threshold`` required) or ``'auto'`` -- masked iff the
    array holds a NaN, decided on the device (``_remap_data_array``'s rule).
    ``host_mask`` (bool array like ``values``, masked mode only): entries to
    treat as missing, as a ``numpy.ma.MaskedArray`` carries them.
    ``limiter`` / ``row_weight``: as :func:`pyremap_amd.engine.remap_tensor`
    takes them.  A limited array takes the whole-array route -- one upload,
    ``engine.remap_tensor``, one download: the pipelines below launch
    ``apply_strided`` on panels, bands and chunks themselves and serve
    ``limiter=None`` only.
    """
    engine.check_limiter(limiter)
    limit = {} if limiter is None else {'limiter': limiter,
                                        'row_weight': row_weight}
    torch = engine.require_gpu()
    device = plan.device
    values = _as_uploadable(values)
    # every route below -- and the pinned result -- is sized from n_a, n_b
    # and the other dims: a field that does not match the mapping stops here
    remap_axes, dst_shape = engine.check_field_extents(
        plan.n_a, plan.n_b, plan.n_b_global, dst_grid_dims, values.shape,
        remap_axes)
    lead = min(remap_axes)
    n_batch = _prod(values.shape[:lead])
    in_place = engine.in_place_addressable(values.shape, remap_axes)
    if mode not in ('fracb', 'masked', 'auto'):
        raise ValueError(f'unknown mode {mode!r}')
    if mode != 'fracb' and threshold is None:
        raise ValueError('the masked branch needs a threshold')
    if mode == 'auto' and want_mask:
        raise ValueError("mode 'auto' answers with NaN-filled data only")
    thr = 0.0 if threshold is None else float(threshold)

    up, down = _side_streams(device)
    main = torch.cuda.current_stream(device)
    host = torch.from_numpy(values)
    # (remap_numpy.py:280-295: the destination dims take the place of the
    # first source axis, every other non-source dim keeps its order -- also
    # the ones BETWEEN two source axes)
    out_shape = list(values.shape[:lead]) + dst_shape + \
        [int(values.shape[ax]) for ax in range(lead, values.ndim)
         if ax not in remap_axes]

    if mode == 'auto' and host_mask is None and values.dtype.kind == 'f' \
            and values.nbytes >= 4 * CHUNK_BYTES and _sampled_nan(values):
        # A NaN was SEEN (a strided sample of the array: microseconds), so
        # the branch is decided -- masked -- before anything is uploaded, and
        # the field takes the pipelined routes below instead of waiting whole
        # on the device for the NaN scan (ocean fields: 36 -> 23 ms per GB).
        # No NaN in the sample decides nothing: the device scan stays.
        mode = 'masked'
    if mode == 'auto' and in_place and n_batch >= 2 and host_mask is None:
        # The branch is decided from the whole array (remap_numpy.py:201-204)
        # and the device-side decision needs the whole array resident.  A
        # series that would not leave HBM room takes the decision on the
        # host instead -- chunk by chunk, stopping at the first NaN (ocean
        # data shows one within the first levels) -- and then streams.
        need = values.nbytes + _prod(out_shape) * 8
        free, _ = torch.cuda.mem_get_info(device)
        if need > DEVICE_FRACTION * free:
            mode = 'masked' if _any_nan(values) else 'fracb'
    if keep_on_device:
        if want_mask or host_mask is not None:
            raise ValueError('keep_on_device answers with NaN-filled data '
                             'of plain arrays only')
        with torch.cuda.device(device):
            x_d = torch.empty(values.shape, dtype=host.dtype, device=device)
            x_d.copy_(host, non_blocking=True)
            if mode == 'auto':
                y_d = engine.remap_tensor_auto_mode(
                    plan, dst_grid_dims, x_d, remap_axes, thr, flags=flags,
                    **limit)
            else:
                emode = engine.MODE_MASKED if mode == 'masked' else \
                    engine.MODE_FRACB
                y_d = engine.remap_tensor(
                    plan, dst_grid_dims, x_d, remap_axes, emode,
                    threshold=thr if emode == engine.MODE_MASKED else 0.0,
                    flags=flags, **limit)
            return OnDevice(y_d, out_shape)
    with torch.cuda.device(device):
        out_h, pin_o = _host_buffer(out_shape, torch.float64)
        mask_h, pin_m = _host_buffer(out_shape, torch.uint8) \
            if want_mask else (None, 0)
        try:
            return _enqueue(plan, dst_grid_dims, values, host, remap_axes,
                            lead, n_batch, in_place, mode, thr, want_mask,
                            flags, host_mask, dst_shape, out_shape, out_h,
                            mask_h, pin_o, pin_m, up, down, main, limit)
        except BaseException:
            # nothing was handed out: the budget goes back
            _release_pinned(pin_o + pin_m)
            raise


def _enqueue(plan, dst_grid_dims, values, host, remap_axes, lead, n_batch,
             in_place, mode, thr, want_mask, flags, host_mask, dst_shape,
             out_shape, out_h, mask_h, pin_o, pin_m, up, down, main,
             limit=None):
    """The transfers and launches of :func:`remap_host_array`."""
    limit = limit or {}
    torch = engine._torch()
    device = plan.device
    # a multi-device plan (parallel.MultiDeviceRemap) shards ROWS over its
    # GPUs per call: one upload to its source device, one sharded remap, one
    # download (the pipelines below drive a single device's launches)
    multi = hasattr(plan, 'shards')
    single = not in_place or host_mask is not None or mode == 'auto' or \
        n_batch < 2 or multi or bool(limit)
    banded = not limit and in_place and host_mask is None and \
        mode != 'auto' and n_batch == 1 and lead == 0 and not multi and \
        values.nbytes >= 4 * CHUNK_BYTES and plan.n_b == plan.n_b_global
    # a field whose source axes lead, (n_a, K): column panels, both PCIe
    # directions busy whatever the mesh numbering (mode 'auto' included:
    # frac_b panel by panel, the masked mode over again if a device scan
    # meets a NaN)
    panels = not limit and in_place and host_mask is None and \
        n_batch == 1 and lead == 0 and not multi and \
        plan.n_b == plan.n_b_global and \
        values.nbytes >= 4 * CHUNK_BYTES and values.flags.c_contiguous and \
        out_h.is_pinned() and (mask_h is None or mask_h.is_pinned())
    if panels:
        got = _panel_pipeline(plan, values, remap_axes, out_h, mask_h, mode,
                              thr, flags, up, down, main)
        if got is not None:
            done, recheck = got
            return Pending(done, out_h, mask_h, (pin_o, pin_m),
                           recheck=recheck)
    # (the batch pipeline below streams through chunk-sized buffers instead)
    x_d = torch.empty(values.shape, dtype=host.dtype, device=device) \
        if single or banded else None
    if banded:
        done = _banded_pipeline(plan, values, remap_axes, host, x_d, out_h,
                                mask_h, mode, thr, flags, up, down, main)
        if done is not None:
            return Pending(done, out_h, mask_h, (pin_o, pin_m))
    if single:
        # ---- one upload, one launch, one download -----------------
        x_d.copy_(host, non_blocking=True)
        poisoned = None
        if host_mask is not None:
            m_d = torch.from_numpy(np.ascontiguousarray(
                host_mask, dtype=np.bool_)).to(device, non_blocking=True)
            # remap_numpy.py:263: matrix.dot(in_mask * in_field) lets an
            # UNMASKED NaN through (NaN * 1) and counts it as valid in
            # the denominator; the kernel, which reads the mask off NaNs,
            # would renormalise it away.  Rare: find out; if so, hand the
            # kernel a finite stand-in there (the denominator -- hence
            # the output mask -- comes out as the reference's) and put
            # the NaNs where the reference has them after the launch.
            poison = torch.isnan(x_d) & ~m_d
            poisoned = poison if bool(poison.any()) else None
            x_d.masked_fill_(m_d, float('nan'))
            if poisoned is not None:
                x_d.masked_fill_(poisoned, 0.0)
        if mode == 'auto':
            y_d = engine.remap_tensor_auto_mode(
                plan, dst_grid_dims, x_d, remap_axes, thr, flags=flags,
                **limit)
            m_out = None
        else:
            emode = engine.MODE_MASKED if mode == 'masked' else \
                engine.MODE_FRACB
            res = engine.remap_tensor(
                plan, dst_grid_dims, x_d, remap_axes, emode,
                threshold=thr if emode == engine.MODE_MASKED else 0.0,
                want_mask=want_mask, flags=flags, **limit)
            y_d, m_out = res if want_mask else (res, None)
        if poisoned is not None:
            # every destination cell that touches a poisoned entry is NaN
            # (and NOT masked) in the reference: 0 * NaN = NaN through a
            # RAW product marks them
            p_field = torch.where(poisoned, float('nan'), 0.0).to(
                torch.float64)
            hit = engine.remap_tensor(plan, dst_grid_dims, p_field,
                                      remap_axes, engine.MODE_RAW,
                                      flags=flags)
            y_d = torch.where(torch.isnan(hit), float('nan'), y_d)
        done = torch.cuda.Event()
        done.record(main)
        with torch.cuda.stream(down):
            down.wait_event(done)
            out_h.copy_(y_d, non_blocking=True)
            if want_mask:
                mask_h.copy_(m_out, non_blocking=True)
            finished = torch.cuda.Event()
            finished.record(down)
        # the device buffers must outlive the copies queued on `down`
        y_d.record_stream(down)
        if m_out is not None:
            m_out.record_stream(down)
        return Pending(finished, out_h, mask_h, (pin_o, pin_m))

    # ---- pipelined: batches of leading dims, three streams ------------
    # Device memory is a RING of chunk-sized buffers, not the whole field:
    # a (Time, nCells, nVertLevels) series larger than HBM streams through
    # (the reference holds it in RAM whole, remap_numpy.py:254-256; the
    # result lives in host memory either way).
    emode = engine.MODE_MASKED if mode == 'masked' else engine.MODE_FRACB
    src_shape = list(values.shape[lead:])
    tail_shape = list(values.shape[lead + len(remap_axes):])
    xb = host.reshape([n_batch] + src_shape)
    ohb = out_h.reshape([n_batch] + dst_shape + tail_shape)
    mhb = mask_h.reshape(ohb.shape) if want_mask else None
    per_batch = max(xb[0].numel() * xb.element_size(), ohb[0].numel() * 8)
    step = max(1, min(n_batch, CHUNK_BYTES // max(per_batch, 1)))
    chunks = [(b0, min(b0 + step, n_batch))
              for b0 in range(0, n_batch, step)]
    ring = min(RING_SLOTS, len(chunks))
    x_slots = [torch.empty([step] + src_shape, dtype=host.dtype,
                           device=device) for _ in range(ring)]
    y_slots = [torch.empty([step] + dst_shape + tail_shape,
                           dtype=torch.float64, device=device)
               for _ in range(ring)]
    m_slots = [torch.empty(y_slots[0].shape, dtype=torch.uint8,
                           device=device) for _ in range(ring)] \
        if want_mask else None
    axes_b = [a - lead + 1 for a in remap_axes]
    start = torch.cuda.Event()
    start.record(main)
    up.wait_event(start)
    finished = None
    # Uploads from PAGEABLE memory block the calling thread until the
    # bytes are on the device, downloads into pinned memory do not: a
    # helper thread feeds the `up` stream so that this thread can queue
    # launches and downloads meanwhile (measured, 0.96 GB up + 1.06 GB
    # down: 22 ms overlapped, 34 ms one after the other)
    # (For fields beyond the CPU caches the host memcpy inside a pageable
    # upload, not PCIe, is the limit: a 7.7 GB series goes up and its 8.5 GB
    # result comes down in 330 ms; see N_UPLOADERS.)
    n_up = min(N_UPLOADERS, len(chunks))
    ups = [up] + [_extra_stream(device, k) for k in range(1, n_up)]
    for st in ups[1:]:
        st.wait_event(start)
    arrivals = [queue.Queue() for _ in range(n_up)]
    consumed = [queue.Queue() for _ in range(n_up)]   # kernel-done events:
    #                                                   an X slot is free

    def uploader(k):
        try:
            with torch.cuda.device(device), torch.cuda.stream(ups[k]):
                for i in range(k, len(chunks), n_up):
                    b0, b1 = chunks[i]
                    if i >= ring:
                        free = consumed[k].get()
                        if free is None:
                            return           # the other side gave up
                        ups[k].wait_event(free)
                    x_slots[i % ring][:b1 - b0].copy_(xb[b0:b1],
                                                      non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(ups[k])
                    arrivals[k].put(ev)
        except BaseException as exc:   # noqa: BLE001 - handed over
            arrivals[k].put(exc)

    feeders = [threading.Thread(target=uploader, args=(k,), daemon=True,
                                name=f'pyremap_amd.ring_uploader_{k}')
               for k in range(n_up)]
    for f in feeders:
        f.start()
    downloaded = []
    try:
        for i, (b0, b1) in enumerate(chunks):
            arrived = arrivals[i % n_up].get()
            if isinstance(arrived, BaseException):
                raise arrived
            n = b1 - b0
            slot = i % ring
            main.wait_event(arrived)
            if i >= ring:
                # the slot's previous result must be on its way out
                main.wait_event(downloaded[i - ring])
            engine.remap_tensor(
                plan, dst_grid_dims, x_slots[slot][:n], axes_b, emode,
                threshold=thr if emode == engine.MODE_MASKED else 0.0,
                want_mask=want_mask, flags=flags, out=y_slots[slot][:n],
                mask_out=m_slots[slot][:n] if want_mask else None)
            computed = torch.cuda.Event()
            computed.record(main)
            # chunk i + ring takes this slot over
            consumed[(i + ring) % n_up].put(computed)
            with torch.cuda.stream(down):
                down.wait_event(computed)
                ohb[b0:b1].copy_(y_slots[slot][:n], non_blocking=True)
                if want_mask:
                    mhb[b0:b1].copy_(m_slots[slot][:n], non_blocking=True)
                finished = torch.cuda.Event()
                finished.record(down)
            downloaded.append(finished)
    except BaseException:
        for q in consumed:
            q.put(None)
        for f in feeders:
            f.join()
        raise
    for f in feeders:
        f.join()
    for st in ups:
        for t in x_slots:
            t.record_stream(st)

    for t in y_slots + (m_slots or []):
        t.record_stream(down)
    return Pending(finished, out_h, mask_h, (pin_o, pin_m))


def _panel_pipeline(plan, values, remap_axes, out_h, mask_h, mode, thr,
                    flags, up, down, main):
    """
    A host field whose source axes lead -- ``(n_a, K)``, what the reference
    flattens every field to (``remap_numpy.py:254-256``) -- in COLUMN PANELS:
    panel p + 1 comes up (one strided 2-D copy straight from the caller's
    pageable array, issued by a feeder thread: such a call holds its thread
    until the bytes are staged) while panel p is remapped and panel p - 1
    goes down into its columns of the pinned result.  Both PCIe directions
    stay busy whatever the numbering of the source mesh (the band pipeline
    needs a numbering no MPAS mesh has): 0.96 GB up + 1.06 GB down in the
    time of the longer of the two plus one panel, not in their sum.

    ``mode='auto'`` (masked iff the field holds a NaN, the reference's rule
    :201-204, and no NaN was seen in the strided sample): the panels are
    remapped in the frac_b mode while a device scan of each looks for NaNs;
    the returned ``recheck`` reads the scans' flag when the result is asked
    for and, should it be set, remaps the (still resident) panels again in
    the masked mode.  Returns ``(event, recheck)`` or ``None`` to decline:
    too few panels, no HIP runtime for the 2-D copies (:func:`_hip`), or
    panels -- source, result and mask stay resident until the result is
    asked for -- beyond ``DEVICE_FRACTION`` of the free device memory.

    The caller has checked the field against the mapping
    (``engine.check_field_extents``); K is the product of the dims behind
    the (leading) source axes.
    """
    torch = engine._torch()
    device = plan.device
    n_a, n_b = plan.n_a, plan.n_b
    K = _prod(values.shape[len(remap_axes):])
    kp = PANEL_COLUMNS
    n_p = (K + kp - 1) // kp
    if n_p < PANEL_MIN or _hip() is None:
        return None
    esize = values.dtype.itemsize
    need = n_p * kp * (n_a * esize + n_b * (9 if mask_h is not None else 8))
    free, _ = torch.cuda.mem_get_info(device)
    if need > DEVICE_FRACTION * free:
        return None
    tdtype = torch.from_numpy(values.reshape(-1)[:0]).dtype
    bounds = [(p * kp, min((p + 1) * kp, K)) for p in range(n_p)]
    x_p = torch.empty((n_p, n_a, kp), dtype=tdtype, device=device)
    y_p = torch.empty((n_p, n_b, kp), dtype=torch.float64, device=device)
    m_p = torch.empty((n_p, n_b, kp), dtype=torch.uint8, device=device) \
        if mask_h is not None else None
    flag = torch.zeros(1, dtype=torch.int32, device=device) \
        if mode == 'auto' else None
    emode = engine.MODE_MASKED if mode == 'masked' else engine.MODE_FRACB
    src = values.ctypes.data
    start = torch.cuda.Event()
    start.record(main)
    up.wait_event(start)
    down.wait_event(start)
    arrivals = queue.Queue()

    def uploader():
        try:
            with torch.cuda.device(device):
                for p, (c0, c1) in enumerate(bounds):
                    _copy_2d(x_p[p].data_ptr(), kp * esize,
                             src + c0 * esize, K * esize, (c1 - c0) * esize,
                             n_a, 1, up)
                    ev = torch.cuda.Event()
                    ev.record(up)
                    arrivals.put(ev)
        except BaseException as exc:   # noqa: BLE001 - handed over
            arrivals.put(exc)

    def launch(p, launch_mode):
        c0, c1 = bounds[p]
        engine.apply_strided(
            plan, x_p[p], y_p[p], n_batch=1, k_inner=c1 - c0,
            x_row_stride=kp, x_batch_stride=0, y_row_stride=kp,
            y_batch_stride=0, mode=launch_mode,
            threshold=thr if launch_mode == engine.MODE_MASKED else 0.0,
            mask_out=m_p[p] if m_p is not None else None, flags=flags)

    def download(p):
        c0, c1 = bounds[p]
        _copy_2d(out_h.data_ptr() + c0 * 8, K * 8, y_p[p].data_ptr(),
                 kp * 8, (c1 - c0) * 8, n_b, 2, down)
        if m_p is not None:
            _copy_2d(mask_h.data_ptr() + c0, K, m_p[p].data_ptr(), kp,
                     c1 - c0, n_b, 2, down)

    feeder = threading.Thread(target=uploader, daemon=True,
                              name='pyremap_amd.panel_uploader')
    feeder.start()
    finished = None
    try:
        for p in range(n_p):
            arrived = arrivals.get()
            if isinstance(arrived, BaseException):
                raise arrived
            main.wait_event(arrived)
            if flag is not None:
                # (a panel whose last columns are not there holds what the
                # allocation held in them: scanned column range only)
                c0, c1 = bounds[p]
                if c1 - c0 == kp:
                    engine.scan_nan(x_p[p], flag)
                else:
                    engine.scan_nan(x_p[p][:, :c1 - c0].contiguous(), flag)
            launch(p, emode)
            computed = torch.cuda.Event()
            computed.record(main)
            down.wait_event(computed)
            download(p)
            finished = torch.cuda.Event()
            finished.record(down)
    except BaseException:
        feeder.join()
        up.synchronize()
        down.synchronize()
        raise
    feeder.join()
    for t in (x_p, y_p) + ((m_p,) if m_p is not None else ()):
        t.record_stream(up)
        t.record_stream(down)
    if flag is None:
        return finished, None
    flag_h = torch.zeros(1, dtype=torch.int32).pin_memory()
    with torch.cuda.stream(down):
        down.wait_stream(main)
        flag_h.copy_(flag, non_blocking=True)
        finished = torch.cuda.Event()
        finished.record(down)

    def recheck():
        if int(flag_h[0]) == 0:
            return
        # a NaN the strided sample did not meet: the reference takes the
        # masked branch for the whole field (remap_numpy.py:201-204) -- the
        # panels are still here
        with torch.cuda.device(device):
            cur = torch.cuda.current_stream(device)
            for p in range(n_p):
                launch(p, engine.MODE_MASKED)
            done = torch.cuda.Event()
            done.record(cur)
            down.wait_event(done)
            for p in range(n_p):
                download(p)
            down.synchronize()
    return finished, recheck


def _banded_pipeline(plan, values, remap_axes, host, x_d, out_h, mask_h, mode,
                     thr, flags, up, down, main):
    """
    A field whose source axes lead -- ``(n_a, K)``, rows contiguous on both
    sides -- with the mode known: X goes up in row chunks, and a block of
    destination rows is launched as soon as the last source row IT references
    has arrived (on a mapping whose destination order follows the source
    mesh that is a band moving through X), its rows going down while later
    chunks still come up.  Both PCIe directions stay busy; every copy is
    contiguous.  Mappings without that locality simply wait for the whole
    upload first (no loss against the plain form).  Returns the event that
    marks the last download, or ``None`` to decline.
    """
    torch = engine._torch()
    device = plan.device
    n_a, n_b = plan.n_a, plan.n_b
    # (the field matches the mapping: engine.check_field_extents in
    # remap_host_array; the source axes lead)
    K = _prod(values.shape[len(remap_axes):])
    if K < 33:
        return None        # the wave-per-row kernels serve partial row ranges
    xh = host.reshape(n_a, K)
    xd = x_d.reshape(n_a, K)
    yh = out_h.reshape(n_b, K)
    mh = mask_h.reshape(n_b, K) if mask_h is not None else None
    y_d = torch.empty((n_b, K), dtype=torch.float64, device=device)
    m_d = torch.empty((n_b, K), dtype=torch.uint8, device=device) \
        if mh is not None else None
    rows_up = max(1, CHUNK_BYTES // (K * xh.element_size()))
    rows_dn = max(1, CHUNK_BYTES // (K * 8))
    ups = [(a, min(a + rows_up, n_a)) for a in range(0, n_a, rows_up)]
    dns = [(r, min(r + rows_dn, n_b)) for r in range(0, n_b, rows_dn)]
    # last source row each destination block needs (one small readback)
    need = plan.block_source_extent(rows_dn)
    if len(need) < 2 or need[len(need) // 2] > 0.9 * n_a:
        # The band only exists when the source mesh is numbered along the
        # destination rows.  No MPAS mesh is (one destination latitude row
        # of the real QU240 mesh meets ids from 77-99 % of the id range), so
        # on a real mapping half the destination blocks need (nearly) every
        # source row: upload whole, launch once, download -- the plain form.
        # Fields with leading batch dims -- (Time, nCells, nVertLevels), the
        # layout MPAS output has -- overlap both directions batch by batch
        # whatever the numbering (the ring pipeline in _enqueue).
        _log_once('banded', 'host array (n_a, K): the source numbering does '
                  'not follow the destination rows; upload, launch and '
                  'download run one after the other')
        return None
    emode = engine.MODE_MASKED if mode == 'masked' else engine.MODE_FRACB
    start = torch.cuda.Event()
    start.record(main)
    up.wait_event(start)
    arrivals = queue.Queue()

    def uploader():
        try:
            with torch.cuda.device(device), torch.cuda.stream(up):
                for a, b in ups:
                    xd[a:b].copy_(xh[a:b], non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(up)
                    arrivals.put((b, ev))
        except BaseException as exc:   # noqa: BLE001 - handed over
            arrivals.put(exc)

    feeder = threading.Thread(target=uploader, daemon=True,
                              name='pyremap_amd.banded_uploader')
    feeder.start()
    have = 0
    finished = None
    for (r0, r1), hi in zip(dns, need):
        while have < hi:
            got = arrivals.get()
            if isinstance(got, BaseException):
                feeder.join()
                raise got
            have, ev = got
            main.wait_event(ev)
        engine.apply_strided(
            plan, xd, y_d, n_batch=1, k_inner=K, x_row_stride=K,
            x_batch_stride=0, y_row_stride=K, y_batch_stride=0, mode=emode,
            threshold=thr if emode == engine.MODE_MASKED else 0.0,
            mask_out=m_d, flags=flags, row_begin=r0, row_end=r1)
        computed = torch.cuda.Event()
        computed.record(main)
        with torch.cuda.stream(down):
            down.wait_event(computed)
            yh[r0:r1].copy_(y_d[r0:r1], non_blocking=True)
            if mh is not None:
                mh[r0:r1].copy_(m_d[r0:r1], non_blocking=True)
            finished = torch.cuda.Event()
            finished.record(down)
    feeder.join()
    x_d.record_stream(up)
    y_d.record_stream(down)
    if m_d is not None:
        m_d.record_stream(down)
    return finished
