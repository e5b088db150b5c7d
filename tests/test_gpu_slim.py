"""SLIM on the device: the coordinate-descent solver (pk_slim_solve_f64) bit for bit against the NumPy restatement of its
contract (tests/slim_reference.py) at the tile edges, on the fixtures, at the sweep cap and on degenerate items, under both
residences of the residual row; the CSR compaction; and the model: batch independence, determinism, the canonical weights,
lists, scores, slices, lifecycle and limits.

The restatement is computed once per input (cached below) and never written to."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import i2i_reference as i2i_ref
import slim_reference as ref
from item_model_helpers import cached_fixture, device_csr as _device_csr, limits_case, model

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 17, 63, 64, 65, 257, 1025, 2050]        # around the wave (64) and the 1024-thread workgroup
RESIDENCES = ['lds', 'global']                         # where the residual row of a column lives


def _device_gram(hip_ops, idx, val, shape, implicit=False):
    """(device image, its host copy [n x n])"""
    G = hip_ops.slim_gram(_device_csr(hip_ops, idx, val, shape, implicit))
    return G, np.ascontiguousarray(hip_ops.to_host(G)[:, :shape[1]])


def _ranges(columns):
    """Sorted columns as (j0, nc) runs."""
    runs = []
    for j in columns:
        if runs and runs[-1][0] + runs[-1][1] == j:
            runs[-1][1] += 1
        else:
            runs.append([j, 1])
    return [tuple(r) for r in runs]


def _device_columns(hip_ops, G, n, columns, l1, l2, tol=1e-4, max_sweeps=100, positive=True):
    """(Wt [len(columns) x n], sweeps) of the listed (sorted) target columns, solved run by run through (j0, nc); checks
    the block's shape and that its pad columns are exactly 0."""
    from polara_amd import slim
    Wt, sweeps = [], []
    for j0, nc in _ranges(columns):
        block, sw = hip_ops.slim_solve(G, n, j0, nc, l1, l2, tol, max_sweeps, positive)
        block = hip_ops.to_host(block)
        assert block.shape == (nc, slim.gram_leading_dim(n)) and not block[:, n:].any()
        Wt.append(block[:, :n])
        sweeps.append(hip_ops.to_host(sw))
    return np.concatenate(Wt), np.concatenate(sweeps)


def _check_columns(Wt, sweeps, Wt_ref, sweeps_ref, columns, positive):
    assert Wt.shape == Wt_ref.shape and sweeps.dtype == np.int32
    assert np.isfinite(Wt).all()
    assert not Wt[np.arange(len(columns)), list(columns)].any()           # w_j[j] == 0
    if positive:
        assert (Wt >= 0).all()
    diff = np.flatnonzero((Wt != Wt_ref).any(axis=1))
    print('%d of %d columns differ; sweeps %s' % (len(diff), len(columns), sorted(set(sweeps.tolist()))))
    assert np.array_equal(sweeps, sweeps_ref)
    assert np.array_equal(Wt, Wt_ref)


# ---- the solver at the tile edges ------------------------------------------------------------------------------------
_EDGE_PENALTIES = {True: (1.0, 5.0), False: (3.0, 20.0)}      # without the sign constraint a larger l1 keeps the solutions sparse
_edge_cache = {}


def _edge_reference(n, positive, Gh):
    if (n, positive) not in _edge_cache:
        cols = list(range(n)) if n < 1025 else [0, 1, n // 2, n - 1]
        Wt, sweeps = ref.solve_columns(Gh, cols, *_EDGE_PENALTIES[positive], positive=positive)
        Wt.setflags(write=False)
        _edge_cache[(n, positive)] = (cols, Wt, sweeps)
    return _edge_cache[(n, positive)]


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('positive', [True, False])
@pytest.mark.parametrize('residence', RESIDENCES)
def test_solver_at_the_tile_edges(n, positive, residence, hip_ops, pk_options):
    if residence == 'global':
        pk_options('slim_r_global', 1)
    idx, val, shape = ref.sized_training(n)
    G, Gh = _device_gram(hip_ops, idx, val, shape)
    assert np.array_equal(Gh, ref.gram(ref.training_matrix(idx, val, shape)))          # integer feedback: exact
    cols, Wt_ref, sweeps_ref = _edge_reference(n, positive, Gh)
    Wt, sweeps = _device_columns(hip_ops, G, n, cols, *_EDGE_PENALTIES[positive], positive=positive)
    _check_columns(Wt, sweeps, Wt_ref, sweeps_ref, cols, positive)
    if n > 2:
        assert np.count_nonzero(Wt) > 0 and sweeps.max() > 1
        assert positive or (Wt < 0).any()


# ---- the fixtures ------------------------------------------------------------------------------------------------------
_fixture = cached_fixture(ref)


def _fixture_columns(name):
    n = ref.FIXTURES[name][1]
    if name != 'large':
        return list(range(n))
    return sorted(np.random.default_rng(40).choice(n, 40, replace=False).tolist())


@functools.lru_cache(maxsize=None)
def _fixture_reference(name, implicit, l1, l2, max_sweeps=100):
    A = _fixture(name, implicit)[3]
    cols = _fixture_columns(name)
    Wt, sweeps = ref.solve_columns(ref.gram(A), cols, l1, l2, 1e-4, max_sweeps)
    Wt.setflags(write=False)
    sweeps.setflags(write=False)
    return cols, Wt, sweeps


@pytest.mark.parametrize('name', sorted(ref.FIXTURES))
@pytest.mark.parametrize('implicit', [False, True])
@pytest.mark.parametrize('l1,l2', ref.PENALTIES)
def test_fixtures_are_bit_equal(name, implicit, l1, l2, hip_ops):
    idx, val, shape, A = _fixture(name, implicit)
    n = shape[1]
    G, Gh = _device_gram(hip_ops, idx, val, shape, implicit)
    assert np.array_equal(Gh, ref.gram(A))
    cols, Wt_ref, sweeps_ref = _fixture_reference(name, implicit, l1, l2)
    assert sweeps_ref.max() <= 38                                           # the cap of 100 does not bind
    Wt, sweeps = _device_columns(hip_ops, G, n, cols, l1, l2)
    _check_columns(Wt, sweeps, Wt_ref, sweeps_ref, cols, True)
    if name == 'small' and implicit and (l1, l2) == (20.0, 50.0):
        assert not Wt.any() and (sweeps == 1).all()                         # the empty-CSR case
        ptr, ind, dat = hip_ops.slim_csr(hip_ops.slim_solve(G, n, 0, n, l1, l2, 1e-4, 100)[0], n)
        assert not hip_ops.to_host(ptr).any() and ind.numel() == 0 and dat.numel() == 0


@pytest.mark.parametrize('residence', RESIDENCES)
def test_the_cap_path(residence, hip_ops, pk_options):
    if residence == 'global':
        pk_options('slim_r_global', 1)
    idx, val, shape, A = _fixture('medium', False)
    n = shape[1]
    G, _ = _device_gram(hip_ops, idx, val, shape)
    cols, Wt_ref, sweeps_ref = _fixture_reference('medium', False, 1.0, 5.0, 3)
    assert (sweeps_ref == 3).sum() > n // 2 and sweeps_ref.max() == 3
    Wt, sweeps = _device_columns(hip_ops, G, n, cols, 1.0, 5.0, max_sweeps=3)
    _check_columns(Wt, sweeps, Wt_ref, sweeps_ref, cols, True)
    _, full, _ = _fixture_reference('medium', False, 1.0, 5.0)
    assert not np.array_equal(full, Wt_ref)                                 # the cap did bind


_EMPTY_ITEM = 57


@functools.lru_cache(maxsize=None)
def _degenerate_input():
    idx, val, shape = ref.training('small')
    keep = idx[:, 1] != _EMPTY_ITEM
    return idx[keep], val[keep], shape


@functools.lru_cache(maxsize=None)
def _degenerate_reference(positive):
    idx, val, shape = _degenerate_input()
    G = ref.gram(ref.training_matrix(idx, val, shape))
    Wt, sweeps = ref.solve_columns(G, range(shape[1]), 1.0, 0.0, positive=positive, max_sweeps=6)
    Wt.setflags(write=False)
    return Wt, sweeps


@pytest.mark.parametrize('positive', [True, False])
@pytest.mark.parametrize('residence', RESIDENCES)
def test_degenerate_items(positive, residence, hip_ops, pk_options):
    """An item without training entries and l2 = 0: den = 0, the coordinate is skipped everywhere; as a target its
    column is empty after one sweep.  No NaN anywhere.  (Six sweeps: the case is about the skipped coordinate.)"""
    if residence == 'global':
        pk_options('slim_r_global', 1)
    idx, val, shape = _degenerate_input()
    n, empty = shape[1], _EMPTY_ITEM
    G, Gh = _device_gram(hip_ops, idx, val, shape)
    assert not Gh[empty].any() and not Gh[:, empty].any()
    cols = list(range(n))
    Wt_ref, sweeps_ref = _degenerate_reference(positive)
    Wt, sweeps = _device_columns(hip_ops, G, n, cols, 1.0, 0.0, positive=positive, max_sweeps=6)
    _check_columns(Wt, sweeps, Wt_ref, sweeps_ref, cols, positive)
    assert not Wt[empty].any() and sweeps[empty] == 1 and not Wt[:, empty].any()


# ---- CSR compaction ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,nc', [(1, 1), (5, 3), (64, 2), (257, 9), (1030, 1100)])
def test_compaction_of_a_block(n, nc, hip_ops):
    """Any dense block: entries != 0 in ascending index order (negative values and a -0.0, which is == 0, included); more
    rows than one chunk of the scan."""
    import torch
    from polara_amd import slim
    rng = np.random.default_rng(n + nc)
    ld = slim.gram_leading_dim(n)
    B = np.where(rng.random((nc, ld)) < 0.3, rng.standard_normal((nc, ld)), 0.0)
    B[:, n:] = 7.0                                                          # beyond n: not part of the rows
    B[0, 0] = -0.0
    if nc > 2:
        B[1] = 0.0                                                          # an empty row
        B[2, :n] = 1.5                                                      # a full row
    ptr, ind, dat = (hip_ops.to_host(x) for x in hip_ops.slim_csr(torch.from_numpy(B).to(hip_ops.device), n))
    want = sps.csr_matrix(B[:, :n])
    want.eliminate_zeros()
    assert ptr.dtype == np.int64 and ind.dtype == np.int32 and dat.dtype == np.float64
    assert np.array_equal(ptr, want.indptr) and np.array_equal(ind, want.indices) and np.array_equal(dat, want.data)


# ---- model ---------------------------------------------------------------------------------------------------------------
def _model(hip_ops, idx, val, shape, test=None, holdout=None, l1=1.0, l2=5.0, implicit=False, **settings):
    return model('SLIMModel', hip_ops, idx, val, shape, test, holdout, l1_regularization=l1, l2_regularization=l2,
                 implicit=implicit, **settings)


def _csr_arrays(hip_ops, W):
    return tuple(hip_ops.to_host(x).copy() for x in (W.indptr, W.indices, W.values))


def _reference_csr(name, implicit=False, l1=1.0, l2=5.0):
    _, Wt_ref, sweeps_ref = _fixture_reference(name, implicit, l1, l2)
    return sps.csr_matrix(np.ascontiguousarray(Wt_ref.T)), sweeps_ref


@pytest.mark.parametrize('residence', RESIDENCES)
def test_item_weights_are_the_canonical_csr_of_the_restatement(residence, hip_ops, pk_options):
    if residence == 'global':
        pk_options('slim_r_global', 1)
    idx, val, shape, _ = _fixture('medium', False)
    n = shape[1]
    m = _model(hip_ops, idx, val, shape)
    m.build()
    W = m.item_weights
    assert W.shape == (n, n) and W.values.dtype.itemsize == 8 and W.indices.dtype.itemsize == 4
    ptr, ind, dat = _csr_arrays(hip_ops, W)
    want, sweeps_ref = _reference_csr('medium')
    assert np.array_equal(ptr, want.indptr) and np.array_equal(ind, want.indices) and np.array_equal(dat, want.data)
    assert (dat != 0).all() and W.nnz == want.nnz == len(dat)
    rows = np.repeat(np.arange(n), np.diff(ptr))
    assert (rows != ind).all()                                              # no diagonal entry
    assert all((np.diff(ind[ptr[r]:ptr[r + 1]]) > 0).all() for r in range(n))        # sorted, no duplicates
    assert m.sweeps.dtype == np.int32 and np.array_equal(m.sweeps, sweeps_ref)
    s = m.build_stats
    assert {'gram_s', 'solve_s', 'csr_s', 'n_items', 'nnz', 'nnz_weights', 'fill', 'max_sweeps', 'mean_sweeps',
            'capped_columns', 'column_batch'} <= set(s)
    assert (s['n_items'], s['nnz'], s['nnz_weights'], s['column_batch']) == (n, len(val), want.nnz, n)
    assert s['fill'] == want.nnz / n ** 2 and s['max_sweeps'] == sweeps_ref.max() and s['capped_columns'] == 0
    assert s['mean_sweeps'] == pytest.approx(sweeps_ref.mean())


def test_batch_independence_and_determinism(hip_ops):
    idx, val, shape, _ = _fixture('small', False)
    n = shape[1]
    m = _model(hip_ops, idx, val, shape)
    results = []
    for batch in (None, 1, 7, n, None):
        m.column_batch = batch
        m.build()
        assert m.build_stats['column_batch'] == (batch or n)
        results.append(_csr_arrays(hip_ops, m.item_weights) + (m.sweeps.copy(),))
    m.build()                                                               # the same settings again
    results.append(_csr_arrays(hip_ops, m.item_weights) + (m.sweeps.copy(),))
    for other in results[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(results[0], other))
    want, sweeps_ref = _reference_csr('small')
    assert np.array_equal(results[0][0], want.indptr) and np.array_equal(results[0][2], want.data)
    assert np.array_equal(results[0][3], sweeps_ref)
    m.max_sweeps = 3
    m.build()
    assert m.build_stats['capped_columns'] == int((m.sweeps == 3).sum()) > 0


def test_empty_weights_model(hip_ops):
    """(l1, l2) = (20, 50) on the signs of `small`: W = 0, an empty CSR; every score is 0."""
    idx, val, shape, _ = _fixture('small', True)
    test, holdout, tshape = ref.test_rows('small')
    m = _model(hip_ops, idx, val, shape, test, holdout, 20.0, 50.0, implicit=True)
    m.topk = 5
    m.build()
    assert m.item_weights.nnz == 0 and not hip_ops.to_host(m.item_weights.indptr).any() and (m.sweeps == 1).all()
    m.filter_seen = False
    assert np.array_equal(m.get_recommendations(), np.tile(np.arange(5), (tshape[0], 1)))        # all tied at 0: item order
    m.dense_output = False
    assert (m.get_recommendations() == -1).all()


@pytest.mark.parametrize('name', ['small', 'medium'])
@pytest.mark.parametrize('implicit', [False, True])
def test_model_lists_and_scores_match_the_restatement(name, implicit, hip_ops):
    idx, val, shape, A = _fixture(name, implicit)
    test, holdout, tshape = ref.test_rows(name)
    m = _model(hip_ops, idx, val, shape, test, holdout, implicit=implicit)
    m.build()
    _, Wt_ref, _ = _fixture_reference(name, implicit, 1.0, 5.0)
    T, seen = i2i_ref.test_matrix(test, tshape, implicit)
    scores = ref.slim_scores(np.ascontiguousarray(Wt_ref.T), T)
    assert not scores[-1].any() and not scores[1].any() and seen[1].any()       # an empty row and a zero-feedback row
    for dense_output in (True, False):
        m.dense_output = dense_output
        for filter_seen in (True, False):
            cls = i2i_ref.classes(scores, seen, filter_seen, not dense_output)
            for topk in (1, 10, 100):
                m.filter_seen, m.topk = filter_seen, topk
                recs = m.get_recommendations()
                want = i2i_ref.select(scores, seen, topk, filter_seen, not dense_output)
                assert recs.shape == want.shape and recs.dtype == np.int64
                assert dense_output == bool((recs >= 0).all())                  # only the sparse branch pads
                # the scoring pass sums in SciPy's order and W is bit-equal: no tolerance, as in test_gpu_sim.py
                assert i2i_ref.tie_aware_mismatches(recs, want, scores, cls, tol=0.0) == [], (dense_output, filter_seen, topk)
                assert np.array_equal(recs, want), (dense_output, filter_seen, topk)
                lists, list_scores = m.recommend_with_scores()
                assert np.array_equal(lists, recs)
                s_ref = np.where(lists >= 0, np.take_along_axis(scores, np.maximum(lists, 0), 1), 0.0)
                assert np.array_equal(list_scores, s_ref), (dense_output, filter_seen, topk)
    assert len(m.training_time) == 1                                            # none of this rebuilt the model
    test_data, test_shape, _ = m._get_test_data()
    block, triplet = m.slice_recommendations(test_data, test_shape, 3, 17)      # the sparse branch: a SciPy CSR
    assert sps.issparse(block) and block.shape == (14, shape[1])
    assert np.array_equal(block.toarray(), scores[3:17]) and (block.data != 0).all()
    m.dense_output = True
    block, triplet = m.slice_recommendations(test_data, test_shape, 3, 17)
    assert isinstance(block, np.ndarray) and np.array_equal(block, scores[3:17])
    assert np.array_equal(triplet[1], test[1][(test[0] >= 3) & (test[0] < 17)])


def test_lifecycle(hip_ops):
    idx, val, shape, _ = _fixture('medium', False)
    test, holdout, tshape = ref.test_rows('medium')
    m = _model(hip_ops, idx, val, shape, test, holdout)
    m.topk = 10
    recs = m.recommendations
    assert recs.shape == (tshape[0], 10) and len(m.training_time) == 1
    m.l1_regularization, m.l2_regularization, m.tolerance, m.positive, m.implicit = 1, 5.0, 1e-4, True, False    # unchanged
    assert m.recommendations is recs and m._is_ready and len(m.training_time) == 1
    m.topk = 20                                                 # growing re-scores, no rebuild
    assert np.array_equal(m.recommendations[:, :10], recs) and len(m.training_time) == 1
    W = m.item_weights
    m.dense_output = False                                      # the other branch: new lists, the same model
    sparse_recs = m.recommendations
    assert m.item_weights is W and len(m.training_time) == 1 and sparse_recs.shape == (tshape[0], 20)
    assert (sparse_recs[-1] == -1).all() and (recs[-1] >= 0).all()          # an empty row: pads only in the sparse branch
    m.dense_output = True
    builds = 1
    for name, value in (('l1_regularization', 5.0), ('l2_regularization', 0.5), ('tolerance', 1e-3), ('positive', False),
                        ('implicit', True)):
        setattr(m, name, value)                                 # a change: the weights are dropped at once, then rebuilt
        assert m.item_weights is None and m.sweeps is None and not m._is_ready, name
        other = m.recommendations
        builds += 1
        assert len(m.training_time) == builds and m.item_weights is not None and other.shape == (tshape[0], 20)
    m.positive, m.implicit, m.tolerance = True, False, 1e-4
    other = m.recommendations
    _, Wt_ref, _ = _fixture_reference('medium', False, 5.0, 0.5)
    T, seen = i2i_ref.test_matrix(test, tshape)
    scores = ref.slim_scores(np.ascontiguousarray(Wt_ref.T), T)
    assert np.array_equal(other, i2i_ref.select(scores, seen, 20, True, False))
    top, seen_items = m.show_recommendations(5, topk=10)
    assert np.array_equal(top, other[5, :10]) and set(seen_items) == set(test[1][test[0] == 5])
    assert m.evaluate(topk=10) is not None
    m.data.set_training_data((idx[:, 0], idx[:, 1], val * 2))    # a data change: a new model
    assert m.item_weights is None and not m._is_ready


def test_stated_limits(hip_ops, monkeypatch):
    from polara_amd import slim
    pairs, val, (n_users, n_items), hold = limits_case()
    m = _model(hip_ops, pairs, val, (n_users, n_items), holdout=hold, l2=slim.DEFAULT_L2, column_batch=7)
    m.topk = 1024
    assert m.recommendations.shape == (n_users, 1024)
    m.topk = 1025
    with pytest.raises(ValueError, match='1024'):
        m.get_recommendations()
    with pytest.raises(ValueError, match='1024'):
        m.recommend_with_scores()
    # the guard speaks before anything is allocated: a fake free-bytes figure, not an exhausted device
    need = slim.gram_image_bytes(n_items) + slim.batch_bytes(n_items, 7)
    monkeypatch.setattr(hip_ops, 'free_bytes', lambda: 2 * need - 16)
    with pytest.raises(MemoryError, match=str(need)):
        m.build()
    assert m.item_weights is None
    monkeypatch.setattr(hip_ops, 'free_bytes', lambda: 2 * need)
    m.build()
    assert m.item_weights is not None
    # more items than the solver takes: the planning function speaks, nothing is allocated
    with pytest.raises(ValueError, match=str(slim.MAX_ITEMS)):
        slim.check_build_memory(hip_ops.lib.pk_slim_max_items() + 1, 1e15)
    monkeypatch.undo()                                          # the device's own free bytes again
    G = hip_ops.slim_gram(hip_ops.csr_from_coo(pairs[:, 0], pairs[:, 1], val, (n_users, n_items)))
    with pytest.raises(ValueError, match='columns'):
        hip_ops.slim_solve(G, n_items, n_items - 1, 2, 1.0, 5.0, 1e-4, 10)
