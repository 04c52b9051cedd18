"""
The five row passes captured in a hipGraph and replayed on NEW data.

``include/remap_hip.h``: "nothing is allocated, freed or synchronised inside
the apply calls, so they are graph-capturable."  tests/test_gpu_graph.py holds
the SpMM apply, the NaN scan and the plan handle to that; here the same is
asked of ``remap_limit_rows`` (behind its apply launch), ``remap_apply_sgs``,
``remap_apply_vector``, ``remap_apply_levels`` and ``remap_apply_layers``
through the strided launchers of the engine: one linear series on one stream,
on fixed device buffers, captured once (torch.cuda.CUDAGraph) and replayed
twice.  The capture itself fails if a launcher allocates, synchronises or
issues on another stream than torch's current one.  Every replay runs on
values that did not exist at capture time, NaNs in other cells; the second
also on other targets, depth ranges and bases written into the captured
tensors: the kernels read them when they run, not when they are issued.

Every comparison is an equality of BYTES with the numpy statements
(``limiter.clip``, ``sgs.apply``, ``vector.apply``, ``levels.apply``,
``layers.apply``; the masked apply in front of the limiter is ``sgs.apply``
with a fraction of one, which tests/test_gpu_sgs.py holds it to).
"""
import numpy as np
import pytest

import layers_cases
import levels_cases
import limiter_cases as cases
import sgs_cases
import vector_cases

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

N_A, N_B = 300, 257
SENTINEL = -7.25e300
NL, B5 = 12, 5
INF = float('inf')
# round 0: the suites' targets and ranges; round 1: another order, a bottom
# at +inf and an empty range, written into the captured tensors
TARGETS = (levels_cases.TARGETS,
           (-5000.0, -12.0, -400.0, -20.0, -150.0, -50.0))
BOUNDS = (layers_cases.BOUNDS,
          ((100.0, 250.0), (20.0, INF), (15.0, 15.0), (0.0, 10.0),
           (5000.0, 6000.0), (390.0, 700.0)))


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).to('cuda:0')


def _flat_strides(k, n_batch=1):
    """``(n_a, k)`` -> ``(n_b, k)``."""
    return dict(n_batch=n_batch, k_inner=k, x_row_stride=k,
                x_batch_stride=N_A * k, y_row_stride=k,
                y_batch_stride=N_B * k)


def _time_strides(B, nl, k, name):
    """``(B, n_a, nl)`` with a time-invariant ``(n_a, 1, nl)`` coordinate or
    thickness -> ``(B, n_b, k)``."""
    return dict({f'{name}_row_stride': nl, f'{name}_batch_stride': 0},
                n_batch=B, n_levels=nl, k_inner=k, x_row_stride=nl,
                x_batch_stride=N_A * nl, y_row_stride=k,
                y_batch_stride=N_B * k)


def _host_inputs(values, tables):
    """The values of one round, as the statements take them: fields of round
    ``values``, targets, ranges and bases of round ``tables``."""
    s = 1000 * (values + 1)
    h = {}
    for k in (3, 64):
        h['limit', k] = cases.field((N_A, k), seed=s + k, nan_share=0.08)
    h['sgs', 3] = (cases.field((N_A, 3), seed=s + 1),
                   sgs_cases.fraction((N_A, 3), seed=s + 2))
    h['sgs', 130] = (cases.field((N_A, 130), np.float32, seed=s + 3),
                     sgs_cases.fraction((N_A, 1), seed=s + 4))
    for key, shape in ((('vector', 1), (N_A, B5)), (('vector', 64),
                                                    (N_A, 64))):
        h[key] = (cases.field(shape, seed=s + 5 + shape[1]),
                  cases.field(shape, seed=s + 6 + shape[1]))
    h['bases'] = (vector_cases.random_basis(N_A, 31 + 2 * tables),
                  vector_cases.random_basis(N_B, 32 + 2 * tables))
    h['levels'] = levels_cases.shared_case(B5, NL, form='time', seed=s + 9)
    h['layers'] = layers_cases.shared_case(B5, NL, form='time', seed=s + 10)
    h['T'] = np.array(TARGETS[tables], dtype=np.float64)
    h['AB'] = np.array(BOUNDS[tables], dtype=np.float64)
    return h


def _expected(h, csr, csr_short):
    """The bytes every output holds after the series."""
    from pyremap_amd import layers, levels, limiter, sgs, vector
    rowptr, col, val = csr
    want = {}
    for k in (3, 64):
        X = h['limit', k]
        applied = sgs.apply(rowptr, col, val, X, np.ones((N_A, 1)), 0.0)[0]
        want['limit', k] = limiter.clip(rowptr, col, X, applied)
    for k in (3, 130):
        X, F = h['sgs', k]
        want['sgs', k] = sgs.apply(rowptr, col, val, X, F, 0.3)[0]
    BA, BB = h['bases']
    for k in (1, 64):
        U, V = h['vector', k]
        want['vector', k] = vector.apply(*csr_short, U, V, BA, BB, 0.3)[:2]
    X, Z = h['levels']
    want['levels'] = levels.apply(rowptr, col, val, X, Z, h['T'], 0.3)[0]
    X, H = h['layers']
    for reduce in ('mean', 'integral'):
        want['layers', reduce] = layers.apply(rowptr, col, val, X, H,
                                              h['AB'], 0.0, reduce)[0]
    return want


def _time_major(a):
    """The statement's ``(n_a, B, nl)`` as the device's ``(B, n_a, nl)``."""
    return np.ascontiguousarray(a.transpose(1, 0, 2))


def test_row_passes_replay_from_a_hip_graph():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from pyremap_amd import engine
    csr = cases.random_case(n_a=N_A, n_b=N_B)
    csr_short = vector_cases.short_case(n_a=N_A, n_b=N_B)
    plan, plan_short = (engine.RemapPlan.from_csr(
        c[0], c[1], c[2], np.ones(N_B), N_A, device='cuda:0')
        for c in (csr, csr_short))
    L, R = len(TARGETS[0]), len(BOUNDS[0])

    def empty(n, dtype=torch.float64):
        return torch.zeros(n, dtype=dtype, device='cuda:0')

    def result(n):
        return torch.full((n,), SENTINEL, dtype=torch.float64,
                          device='cuda:0')
    # every buffer of the series, allocated in front of the capture
    d = {('limit', k): empty(N_A * k) for k in (3, 64)}
    d['sgs', 3] = (empty(N_A * 3), empty(N_A * 3))
    d['sgs', 130] = (empty(N_A * 130, torch.float32), empty(N_A))
    d['vector', 1] = (empty(B5 * N_A), empty(B5 * N_A))
    d['vector', 64] = (empty(N_A * 64), empty(N_A * 64))
    d['bases'] = (empty(N_A * 5).reshape(N_A, 5),
                  empty(N_B * 5).reshape(N_B, 5))
    d['levels'] = (empty(B5 * N_A * NL), empty(N_A * NL))
    d['layers'] = (empty(B5 * N_A * NL), empty(N_A * NL))
    d['T'], d['AB'] = empty(L), empty(R * 2)
    out = {('limit', k): tuple(result(N_B * k) for _ in range(3))
           for k in (3, 64)}
    out.update({('sgs', k): result(N_B * k) for k in (3, 130)})
    out['vector', 1] = (result(B5 * N_B), result(B5 * N_B))
    out['vector', 64] = (result(N_B * 64), result(N_B * 64))
    out['levels'] = result(B5 * N_B * L)
    out.update({('layers', r): result(B5 * N_B * R)
                for r in ('mean', 'integral')})

    def upload(h):
        for k in (3, 64):
            d['limit', k].copy_(_dev(h['limit', k]).reshape(-1))
        for key in (('sgs', 3), ('sgs', 130), ('vector', 64)):
            for t, a in zip(d[key], h[key]):
                t.copy_(_dev(a).reshape(-1))
        for t, a in zip(d['vector', 1], h['vector', 1]):
            t.copy_(_dev(a.T).reshape(-1))              # (B, n_a, 1)
        for t, a in zip(d['bases'], h['bases']):
            t.copy_(_dev(a))
        for key in ('levels', 'layers'):
            X, Z = h[key]
            d[key][0].copy_(_dev(_time_major(X)).reshape(-1))
            d[key][1].copy_(_dev(Z).reshape(-1))        # (n_a, 1, nl)
        d['T'].copy_(_dev(h['T']))
        d['AB'].copy_(_dev(h['AB']).reshape(-1))

    def series():
        for k in (3, 64):           # rowlane; rowwave, two columns a lane
            y, lo, hi = out['limit', k]
            engine.apply_strided(plan, d['limit', k], y,
                                 mode=engine.MODE_MASKED, threshold=0.0,
                                 **_flat_strides(k))
            engine.limit_strided(plan, d['limit', k], y, lo=lo, hi=hi,
                                 **_flat_strides(k))
        engine.sgs_strided(plan, *d['sgs', 3], out['sgs', 3], threshold=0.3,
                           f_row_stride=3, f_batch_stride=N_A * 3,
                           f_inner_stride=1, **_flat_strides(3))
        engine.sgs_strided(plan, *d['sgs', 130], out['sgs', 130],
                           threshold=0.3, f_row_stride=1, f_batch_stride=N_A,
                           f_inner_stride=0, **_flat_strides(130))
        engine.vector_strided(plan_short, *d['vector', 1], *d['bases'],
                              *out['vector', 1], threshold=0.3, n_batch=B5,
                              k_inner=1, x_row_stride=1, x_batch_stride=N_A,
                              y_row_stride=1, y_batch_stride=N_B)
        engine.vector_strided(plan_short, *d['vector', 64], *d['bases'],
                              *out['vector', 64], threshold=0.3,
                              **_flat_strides(64))
        engine.levels_strided(plan, *d['levels'], d['T'], out['levels'],
                              threshold=0.3, **_time_strides(B5, NL, L, 'z'))
        for reduce in ('mean', 'integral'):
            engine.layers_strided(plan, *d['layers'], d['AB'],
                                  out['layers', reduce], threshold=0.0,
                                  reduce=reduce,
                                  **_time_strides(B5, NL, R, 'h'))

    def outputs():
        return [t for v in out.values()
                for t in (v if isinstance(v, tuple) else (v,))]

    def check(h, what):
        want = _expected(h, csr, csr_short)
        got = {key: tuple(t.cpu().numpy() for t in v)
               if isinstance(v, tuple) else v.cpu().numpy()
               for key, v in out.items()}
        for k in (3, 64):
            for g, w, name in zip(got['limit', k], want['limit', k],
                                  ('Y', 'lo', 'hi')):
                assert cases.same_bytes(g.reshape(N_B, k), w), \
                    (what, 'limit', k, name)
            assert np.isnan(want['limit', k][0]).any()
        for k in (3, 130):
            assert cases.same_bytes(got['sgs', k].reshape(N_B, k),
                                    want['sgs', k]), (what, 'sgs', k)
        for g, w in zip(got['vector', 1], want['vector', 1]):
            assert cases.same_bytes(g.reshape(B5, N_B).T, w), \
                (what, 'vector', 1)
        for g, w in zip(got['vector', 64], want['vector', 64]):
            assert cases.same_bytes(g.reshape(N_B, 64), w), \
                (what, 'vector', 64)
        assert cases.same_bytes(
            got['levels'].reshape(B5, N_B, L).transpose(1, 0, 2),
            want['levels']), (what, 'levels')
        for reduce in ('mean', 'integral'):
            assert cases.same_bytes(
                got['layers', reduce].reshape(B5, N_B, R).transpose(1, 0, 2),
                want['layers', reduce]), (what, 'layers', reduce)
        for key in (('sgs', 3), ('sgs', 130), 'levels', ('layers', 'mean'),
                    ('layers', 'integral')):
            assert np.isnan(want[key]).any() and \
                not np.isnan(want[key]).all(), key
        for w in want['vector', 1] + want['vector', 64]:
            assert np.isnan(w).any() and not np.isnan(w).all()
        return want

    # an eager pass first: whatever a launcher builds on first use
    h0 = _host_inputs(0, 0)
    upload(h0)
    series()
    torch.cuda.synchronize()
    first = check(h0, 'eager')
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        series()
    seen = [first]
    for round_ in (0, 1):
        # new fields every round; the second also rewrites the targets, the
        # ranges and the two bases in the captured tensors
        h = _host_inputs(round_ + 1, round_)
        upload(h)
        for t in outputs():
            t.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        seen.append(check(h, f'replay {round_}'))
    # the rounds asked for different bytes
    for key in seen[0]:
        a, b, c = (np.asarray(s[key]) for s in seen)
        assert not cases.same_bytes(a, b) and not cases.same_bytes(b, c), key
