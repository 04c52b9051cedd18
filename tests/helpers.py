"""Shared helpers for the parity tests."""
import glob
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')

#: unit roundoff of float64
U = 2.0 ** -53


def oracle_threads():
    """Host threads for the CPU oracle: OMP_NUM_THREADS when it is set,
    else at most 16 (one test command's share of a large host)."""
    try:
        n = int(os.environ.get('OMP_NUM_THREADS', ''))
    except ValueError:
        n = 0
    return n if n > 0 else min(16, os.cpu_count() or 1)


def golden_files(pattern='g[01256]_*.npz'):
    return sorted(glob.glob(os.path.join(GOLDEN, pattern)))


def assert_bitwise(actual, expected, what=''):
    """
    Bit-exact comparison for fp64 results: identical NaN placement, and
    identical bit patterns (sign of zero included) everywhere else.  NaN
    payloads are not compared (x86 and gfx950 pick different default NaNs).
    """
    actual = np.ascontiguousarray(actual, dtype=np.float64)
    expected = np.ascontiguousarray(expected, dtype=np.float64)
    assert actual.shape == expected.shape, \
        f'{what}: shape {actual.shape} != {expected.shape}'
    nan_a = np.isnan(actual)
    nan_e = np.isnan(expected)
    assert np.array_equal(nan_a, nan_e), \
        f'{what}: NaN placement differs at {np.argwhere(nan_a != nan_e)[:5]}'
    bits_a = actual.view(np.int64)[~nan_a]
    bits_e = expected.view(np.int64)[~nan_e]
    bad = bits_a != bits_e
    if bad.any():
        idx = np.flatnonzero(bad)[:5]
        raise AssertionError(
            f'{what}: {bad.sum()} of {bad.size} values differ bitwise, e.g. '
            f'{actual[~nan_a][idx]} vs {expected[~nan_e][idx]}')


def golden_cases(path):
    """Yield (index, field-as-handed-over, remap_axes, thr, out, mask)."""
    g = np.load(path)
    for i in range(int(g['n_cases'])):
        field = g[f'c{i}_field']
        thr = float(g[f'c{i}_thr'])
        thr = None if np.isnan(thr) else thr
        if f'c{i}_in_mask' in g:
            arg = np.ma.masked_array(field, g[f'c{i}_in_mask'])
        elif bool(g[f'c{i}_was_masked_array']):
            arg = np.ma.masked_array(field, np.isnan(field))
        else:
            arg = field
        yield (i, arg, [int(a) for a in g[f'c{i}_remap_axes']], thr,
               g[f'c{i}_out'], g[f'c{i}_mask'])


def golden_map(path):
    g = np.load(path)
    return {k: g[k] for k in ('n_a', 'n_b', 'src_grid_dims', 'dst_grid_dims',
                              'row', 'col', 'S', 'frac_b', 'csr_indptr',
                              'csr_indices', 'csr_data')}


def reference_group_schedule(plan, grid_dims=None, super_tile=32, rows=8):
    """
    The row-group schedule of kernel family 10 written out with plain torch
    operations on the host's view of the CSR -- an independent restatement of
    what ``remap_groups_build`` (csrc/remap_schedule.hip) produces on the
    device: ``(meta, col, mask, w, rid, frac, order, n_union)``.
    """
    import torch
    G = int(rows)
    gx = G // 2
    dev = plan.device
    if grid_dims is not None and len(grid_dims) == 2:
        my, mx = (int(d) for d in grid_dims)
        st = int(super_tile) if super_tile and super_tile < 1 << 30 \
            else 1 << 30
        r = torch.arange(plan.row_offset, plan.row_offset + plan.n_b,
                         device=dev, dtype=torch.int64)
        jy = r // mx
        jx = r - jy * mx
        nsx = (mx + st - 1) // st
        key = ((jy // st) * nsx + jx // st) * (st * st) + \
            (((jy % st) // 2) * (st // gx) + (jx % st) // gx) * G + \
            (jy % 2) * gx + jx % gx
        order = torch.argsort(key, stable=True).to(torch.int32)
        slot_of_row = torch.empty(plan.n_b, dtype=torch.int64, device=dev)
        slot_of_row[order.to(torch.int64)] = torch.arange(plan.n_b,
                                                          device=dev)
    else:
        order = None
        slot_of_row = torch.arange(plan.n_b, device=dev)
    lens = plan.rowptr[1:] - plan.rowptr[:-1]
    entry_slot = torch.repeat_interleave(slot_of_row, lens)
    group_of_entry = entry_slot // G
    member = entry_slot % G
    n_groups = (plan.n_b + G - 1) // G
    key = group_of_entry * plan.n_a + plan.col.to(torch.int64)
    uniq, inverse = torch.unique(key, sorted=True, return_inverse=True)
    nu = int(uniq.shape[0])
    meta = torch.zeros((n_groups + 1, 2), dtype=torch.int64, device=dev)
    meta[1:, 0] = torch.cumsum(torch.bincount(uniq // plan.n_a,
                                              minlength=n_groups), 0)
    meta[1:, 1] = torch.cumsum(torch.bincount(group_of_entry,
                                              minlength=n_groups), 0)
    perm = torch.argsort(inverse * G + member)
    w = plan.val[perm]
    mask = torch.zeros(nu, dtype=torch.int32, device=dev)
    mask.index_add_(0, inverse, (1 << member).to(torch.int32))
    col = (uniq % plan.n_a).to(torch.int32)
    rid = torch.full((n_groups * G,), max(plan.n_b - 1, 0),
                     dtype=torch.int32, device=dev)
    rid[:plan.n_b] = order if order is not None else torch.arange(
        plan.n_b, device=dev, dtype=torch.int32)
    frac = plan.frac_b[rid.to(torch.int64)]
    return meta, col, mask, w, rid, frac, order, nu


def reference_patch_plan(plan, grid_dims, tile, rows_hint=None):
    """
    The LDS patch plan of kernel family 5 for a FIXED tile, written out with
    plain torch operations -- an independent restatement of what
    ``remap_patches_build`` (csrc/remap_schedule.hip) produces on the device:
    ``(ptr, ucol, rowptr, lidx, val, order, distinct, umax, emax)``.
    """
    import torch
    dev = plan.device
    ty, tx = (int(t) for t in tile)
    lens = plan.rowptr[1:] - plan.rowptr[:-1]
    entry_row = torch.repeat_interleave(
        torch.arange(plan.n_b, device=dev), lens)
    col64 = plan.col.to(torch.int64)
    if grid_dims is not None and len(grid_dims) == 2:
        my, mx = (int(d) for d in grid_dims)
        r = torch.arange(plan.row_offset, plan.row_offset + plan.n_b,
                         device=dev, dtype=torch.int64)
        jy = r // mx
        jx = r - jy * mx
        ntx = (mx + tx - 1) // tx
        key = ((jy // ty) * ntx + jx // tx) * (ty * tx) + \
            (jy % ty) * tx + jx % tx
        order = torch.argsort(key, stable=True).to(torch.int32)
        slot_of_row = torch.empty(plan.n_b, dtype=torch.int64, device=dev)
        slot_of_row[order.to(torch.int64)] = torch.arange(plan.n_b,
                                                          device=dev)
    else:
        order = None
        slot_of_row = torch.arange(plan.n_b, device=dev)
    rows = ty * tx
    n_patches = (plan.n_b + rows - 1) // rows
    patch_of_entry = slot_of_row[entry_row] // rows
    key = patch_of_entry * plan.n_a + col64
    uniq, inverse = torch.unique(key, sorted=True, return_inverse=True)
    counts = torch.bincount(uniq // plan.n_a, minlength=n_patches)
    ptr = torch.zeros(n_patches + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(counts, 0)
    lidx = (inverse - ptr[patch_of_entry]).to(torch.int32)
    rows_by_slot = order.to(torch.int64) if order is not None else \
        torch.arange(plan.n_b, device=dev)
    lens_by_slot = lens[rows_by_slot]
    prow = torch.zeros(plan.n_b + 1, dtype=torch.int64, device=dev)
    prow[1:] = torch.cumsum(lens_by_slot, 0)
    shift = plan.rowptr[:-1][rows_by_slot] - prow[:-1]
    src = torch.repeat_interleave(shift, lens_by_slot) + \
        torch.arange(plan.nnz, device=dev)
    per_patch = prow[torch.arange(0, n_patches * rows + 1, rows,
                                  device=dev).clamp(max=plan.n_b)]
    return (ptr.to(torch.int32), (uniq % plan.n_a).to(torch.int32),
            prow.to(torch.int32), lidx[src], plan.val[src], order,
            int(uniq.shape[0]), int(counts.max()),
            int((per_patch[1:] - per_patch[:-1]).max()))


# ---------------------------------------------------------------------------
# a sound check for the sums that are not bit-exact (REMAP_FLAG_FMA / TREE)
# ---------------------------------------------------------------------------

def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a            # 2**27 + 1: Dekker's splitter
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, ah, al, b):
    """a * b = p + e exactly (Dekker; a's halves ah + al given)."""
    p = a * b
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_rows(indptr, indices, data, X, masked, r0, r1):
    """
    Rows r0..r1 of the CSR against X (n_cols, K): num = sum S v x and
    den = sum S v as double-doubles (Ogita-Rump-Oishi Dot2, vectorised
    across the K columns; v = 1, or 0 where x is NaN in the masked mode),
    plus sum |S v x|, sum |S v| and the row lengths.
    """
    R, K = r1 - r0, X.shape[1]
    lens = (indptr[r0 + 1:r1 + 1] - indptr[r0:r1]).astype(np.int64)
    nh = np.zeros((R, K))
    nl = np.zeros((R, K))
    dh = np.zeros((R, K))
    dl = np.zeros((R, K))
    absn = np.zeros((R, K))
    absd = np.zeros((R, K))
    for j in range(int(lens.max(initial=0))):
        live = lens > j
        at = np.where(live, indptr[r0:r1] + j, 0)
        w = np.where(live, data[at] if len(data) else 0.0, 0.0)[:, None]
        x = X[indices[at] if len(indices) else np.zeros(R, np.int64)]
        x = np.where(live[:, None], x, 0.0)
        if masked:
            v = ~np.isnan(x)
            x = np.where(v, x, 0.0)
            wv = np.where(v, w, 0.0)
        else:
            wv = np.broadcast_to(w, (R, K))
        wh, wl = _split(w)
        p, e = _two_prod(w, wh, wl, x)
        nh, q = _two_sum(nh, p)
        nl = nl + (q + e)
        dh, q = _two_sum(dh, wv)
        dl = dl + q
        absn = absn + np.abs(p)
        absd = absd + np.abs(wv)
    nh, nl = _two_sum(nh, nl)
    dh, dl = _two_sum(dh, dl)
    return nh, nl, dh, dl, absn, absd, lens


def _dd_div(nh, nl, dh, dl):
    """(nh + nl) / (dh + dl) rounded to float64 (error O(u^2) relative)."""
    with np.errstate(divide='ignore', invalid='ignore'):
        q1 = nh / dh
        dh_h, dh_l = _split(dh)
        p, e = _two_prod(dh, dh_h, dh_l, q1)
        r = (((nh - p) - e) + nl) - q1 * dl
        return q1 + r / dh


def check_sum_bound(csr, frac_b, X, got, mode, thr=0.0, got_mask=None,
                    what='', nthreads=None, block=256):
    """
    Check a remap result whose sums may be associated in ANY order, with or
    without fused multiply-adds, against a double-double reference.

    ``csr`` (an ``oracle.OracleCSR``; a row sub-CSR with compacted columns
    will do), ``frac_b`` (its rows), ``X`` (n_cols, K) float64, ``got``
    (n_rows, K) with NaN where masked; ``mode`` 'raw', 'fracb' or 'masked'
    (``thr``: the renormalisation threshold); ``got_mask`` the kernel's mask
    (True = masked), if it returned one.

    Reference: num = sum S v x and den (``frac_b``, or sum S v in the masked
    mode, v = 0 where x is NaN, else 1) in double-double, ref = num / den.

    Bound, per element of a row of n entries, u = 2**-53, g_k = k u / (1 -
    k u), A = sum |S v x|, B = sum |S v| (B = 0 in the frac_b mode, where den
    is exact; the raw mode has den = 1):

        |got - ref| <= g_{n+1} (A + |ref| B) / |den| + 3 u |ref|

    Derivation.  Any summation of n terms, in any order, with or without
    fused multiply-adds, gives num' = num + e_n, |e_n| <= g_n A (Higham,
    Accuracy and Stability, 2nd ed., (3.5) and its remark on the order;
    an FMA only drops a rounding).  v is 0 or 1, so S v is exact and den' =
    den + e_d, |e_d| <= g_n B.  got = num' / den' (1 + d), |d| <= u, so

        got - ref = (e_n - ref e_d) / den' (1 + d) + ref d,
        |got - ref| <= g_n (A + |ref| B) / |den| (1 + u) / (1 - h) + u |ref|

    with h = g_n B / |den|.  While h <= 1 / (n + 1), g_n (1 + u) / (1 - h)
    <= g_{n+1}, the bound above; rows where h is larger use the middle line
    itself (and accept anything when h >= 1: den's sign is not known).  The
    reference is num / den rounded once (<= u |ref|) with a double-double
    error of O(n u^2) relative to A / |den|: the remaining u |ref| covers it.

    The mask (den > thr in the masked mode, frac_b > 0 otherwise) and the
    placement of NaN must match exactly, except in rows whose |den - thr|
    lies within den's own bound g_n B: either answer is accepted there.
    Returns the largest |got - ref| / bound seen.
    """
    from concurrent.futures import ThreadPoolExecutor
    got = np.asarray(got, dtype=np.float64)
    X = np.ascontiguousarray(X, dtype=np.float64)
    n_rows, K = got.shape
    assert X.shape[1] == K, what
    indptr = np.asarray(csr.indptr, dtype=np.int64)
    indices = np.asarray(csr.indices, dtype=np.int64)
    data = np.asarray(csr.data, dtype=np.float64)
    frac_b = np.asarray(frac_b, dtype=np.float64)
    masked = mode == 'masked'

    def one(r0):
        r1 = min(r0 + block, n_rows)
        nh, nl, dh, dl, A, B, lens = _dd_rows(indptr, indices, data, X,
                                               masked, r0, r1)
        n = lens[:, None].astype(np.float64)
        g_n = n * U / (1 - n * U)
        g_n1 = (n + 1) * U / (1 - (n + 1) * U)
        if mode == 'masked':
            den = dh + dl
            ref = _dd_div(nh, nl, dh, dl)
            ok = den > thr
            unsure = np.abs(den - thr) <= g_n * B
        else:
            den = np.broadcast_to((frac_b[r0:r1] if mode == 'fracb' else
                                   np.ones(r1 - r0))[:, None], nh.shape)
            ref = _dd_div(nh, nl, den, 0.0)
            ok = den > 0.0 if mode == 'fracb' else np.ones(nh.shape, bool)
            B = np.zeros_like(B)
            unsure = np.zeros(nh.shape, bool)
        # (A and B were summed in float64 themselves: a factor 1 + g_n)
        A = A * (1 + 2 * g_n)
        B = B * (1 + 2 * g_n)
        g = got[r0:r1]
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            ad = np.abs(den)
            e = g_n * (A + np.abs(ref) * B)
            h = g_n * B / ad
            general = np.where(h < 1, e * (1 + U) / (ad * (1 - h)), np.inf)
            bound = np.maximum(g_n1 * (A + np.abs(ref) * B) / ad,
                               general) + 3 * U * np.abs(ref)
        want_nan = ~ok | np.isnan(ref)
        bad = (np.isnan(g) != want_nan) & ~unsure
        if bad.any():
            i, k = np.argwhere(bad)[0]
            raise AssertionError(
                f'{what}: NaN placement differs at row {r0 + i} column {k} '
                f'({bad.sum()} elements): got {g[i, k]}, ref {ref[i, k]}, '
                f'den {den[i, k]}')
        if got_mask is not None:
            gm = np.asarray(got_mask[r0:r1]).astype(bool)
            badm = (gm != ~ok) & ~unsure
            assert not badm.any(), \
                f'{what}: mask differs at {np.argwhere(badm)[:3] + [r0, 0]}'
        fin = ~np.isnan(g) & ~np.isnan(ref) & (ok | unsure)
        err = np.where(fin, np.abs(g - ref), 0.0)
        over = err > bound
        if over.any():
            i, k = np.argwhere(over)[0]
            raise AssertionError(
                f'{what}: {over.sum()} values outside the summation bound, '
                f'e.g. row {r0 + i} column {k}: got {g[i, k]!r}, ref '
                f'{ref[i, k]!r}, |err| {err[i, k]:.3e} > bound '
                f'{bound[i, k]:.3e}')
        with np.errstate(invalid='ignore'):
            ratio = np.where(fin & (bound > 0), err / bound, 0.0)
        return float(ratio.max(initial=0.0))

    threads = nthreads or oracle_threads()
    starts = range(0, n_rows, block)
    if threads <= 1 or n_rows <= block:
        return max((one(r0) for r0 in starts), default=0.0)
    with ThreadPoolExecutor(threads) as pool:
        return max(pool.map(one, starts), default=0.0)
