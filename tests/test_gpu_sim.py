"""The sparse x sparse product with the fused top-k (csrc/simagg.hip) and the two models on it, on the device: the dense
rows against SciPy's product BIT FOR BIT (the kernel's contract: the summation order of csr_matmat, separate multiply and
add), the lists against `i2i_reference.select` exactly, the models against the reference's lists of tests/golden (tie-aware,
tolerance 0) and against the restatement of tests/sim_reference.py, determinism, argument checks and the model lifecycle."""
import numpy as np
import pytest
import scipy.sparse as sps

import i2i_reference as ref
import sim_reference as sim
from conftest import GoldenData, load_golden

pytestmark = pytest.mark.gpu

SIM_FIXTURES = ['sim_sparse', 'sim_nofilter', 'sim_warm', 'sim_implicit', 'sim_dense', 'sim_nonsym']
SIMCS_FIXTURES = ['simcs_sparse', 'simcs_full', 'simcs_implicit']


# ---- seeded operands ---------------------------------------------------------------------------------------------------
def _operands(case):
    """(L, B) SciPy CSR, canonical: every path of the kernel at the smallest shapes that reach it (see CASES)."""
    n_inner, n_cols, step = CASES[case]
    rng = np.random.default_rng(500 + case)

    def values(k, signed=True):
        v = rng.integers(1, 30, k) * step
        return np.where(rng.random(k) < 0.3, -v, v) if signed else v

    # ---- B: empty rows, a full row, a row with > 64 entries inside one 512-column quarter, rows cut by the edges ----
    b_rows = []
    edge = np.array([c for c in (0, 511, 512, 1023, 1024, 2047, 2048, 2049, 4095, 4096) if c < n_cols])
    for i in range(n_inner):
        kind = i % 11
        if kind == 0:
            cols = np.zeros(0, dtype=np.int64)                              # empty row
        elif i == 1:
            cols = np.arange(n_cols)                                        # one full row
        elif kind == 2:
            cols = np.arange(min(n_cols, 3), min(n_cols, 3 + 150))          # 150 entries inside the first quarter
        elif kind == 3:
            cols = edge                                                     # 511 | 512, 2047 | 2048: quarter and window edges
        elif kind == 4:
            cols = np.unique(np.r_[edge, rng.choice(n_cols, 5)])
        else:
            cols = np.sort(rng.choice(n_cols, min(n_cols, int(rng.integers(1, 12))), replace=False))
        b_rows.append((cols, values(len(cols))))
    # rows 5 and 6 of B are equal: +v and -v on them cancel exactly
    b_rows[6] = (b_rows[5][0].copy(), b_rows[5][1].copy())
    b_indptr = np.r_[0, np.cumsum([len(c) for c, _ in b_rows])]
    B = sps.csr_matrix((np.concatenate([v for _, v in b_rows]), np.concatenate([c for c, _ in b_rows]), b_indptr),
                       shape=(n_inner, n_cols))

    # ---- L: empty, zeros only, the batch edges 64 / 65 / 130, an exact cancellation, one heavy row, short rows ----------
    def row(k):
        return np.sort(rng.choice(n_inner, min(n_inner, k), replace=False))
    l_rows = [(np.zeros(0, dtype=np.int64), np.zeros(0)),
              (row(7), np.zeros(7)),
              (np.array([5, 6]), np.array([7 * step, -7 * step])),
              (row(64), values(64)), (row(65), values(65)), (row(130), values(130)),
              (row(int(0.6 * n_inner)), values(int(0.6 * n_inner)))]
    for _ in range(5):
        k = int(rng.integers(1, 20))
        l_rows.append((row(k), values(k)))
    l_rows.append((np.array([0]), np.array([3 * step])))                 # meets only an empty row of B
    l_indptr = np.r_[0, np.cumsum([len(c) for c, _ in l_rows])]
    L = sps.csr_matrix((np.concatenate([v for _, v in l_rows]), np.concatenate([c for c, _ in l_rows]), l_indptr),
                       shape=(len(l_rows), n_inner))
    assert L.has_canonical_format and B.has_canonical_format
    return L, B


CASES = [  # (n_inner, n_cols, value step)
    (300, 300, 0.1),        # one window, far from full
    (1030, 1030, 1.0 / 3),  # one window, three quarters in use
    (2048, 2048, 0.1),      # exactly one window
    (2049, 2049, 1.0),      # one column over; integer values: L travels as fp32
    (4500, 4500, 0.1),      # several windows
    (6200, 6200, 1.0 / 3),  # ragged last lane group of the last window
    (700, 4500, 0.1),       # rectangular, n_inner < n_cols
    (2500, 300, 1.0 / 3),   # rectangular, n_inner > n_cols
]


def _device(hip_ops, M):
    return hip_ops.csr(M.indptr, M.indices, M.data, M.shape)


@pytest.fixture(scope='module')
def operands(hip_ops):
    """Per case: (L, B, SciPy's product, seen mask, device L, device B) — computed once, never written."""
    out = []
    for case in range(len(CASES)):
        L, B = _operands(case)
        scores = sim.product(L, B)
        scores.setflags(write=False)
        seen = sim.seen_mask(L) if L.shape[1] == B.shape[1] else None
        out.append((L, B, scores, seen, _device(hip_ops, L), _device(hip_ops, B)))
    return out


@pytest.mark.parametrize('case', range(len(CASES)))
def test_rows_are_bit_equal_to_scipy(case, hip_ops, operands):
    L, B, scores, _, Ld, Bd = operands[case]
    assert (scores[2] == 0).all() and np.count_nonzero(scores) > 0         # the exact cancellation is in the case
    if CASES[case][2] == 1.0:
        assert Ld.values.dtype.itemsize == 4
    got = hip_ops.spsp_rows(Ld, Bd).cpu().numpy()
    assert got.shape == scores.shape and got.dtype == np.float64
    diff = np.flatnonzero((got != scores).ravel())
    print('case %d: %d of %d entries differ' % (case, len(diff), scores.size))
    assert np.array_equal(got, scores)
    assert not np.signbit(got[got == 0]).any()
    part = hip_ops.spsp_rows(Ld, Bd, rows=(3, 7)).cpu().numpy()
    assert np.array_equal(part, scores[3:7])


def test_reverse_order_would_not_pass():
    """The comparison above has teeth: the same products summed in descending order differ from SciPy's in the last bits."""
    L, B = _operands(4)
    fwd = sim.product(L, B)
    Lr = L.copy()
    rev = np.zeros_like(fwd)
    for r in range(L.shape[0]):
        lo, hi = Lr.indptr[r], Lr.indptr[r + 1]
        for p in range(hi - 1, lo - 1, -1):
            i, v = Lr.indices[p], Lr.data[p]
            cols = B.indices[B.indptr[i]:B.indptr[i + 1]]
            rev[r, cols] += v * B.data[B.indptr[i]:B.indptr[i + 1]]
    assert np.allclose(rev, fwd, rtol=1e-12, atol=1e-12) and not np.array_equal(rev, fwd)


@pytest.mark.parametrize('case', range(len(CASES)))
def test_topk_equals_select(case, hip_ops, operands):
    L, B, scores, seen, Ld, Bd = operands[case]
    square = seen is not None
    none_seen = np.zeros(scores.shape, dtype=bool)
    for topk in (1, 10, 100, 1024):
        for sparse in (True, False):
            for filter_seen in ((True, False) if square else (False,)):
                mask = seen if filter_seen else none_seen
                want = ref.select(scores, mask, topk, filter_seen, sparse)
                got, got_s = hip_ops.spsp_topk(Ld, Bd, topk, filter_seen, sparse, want_scores=True)
                got, got_s = got.cpu().numpy(), got_s.cpu().numpy()
                assert np.array_equal(got, want), (topk, sparse, filter_seen)
                live = got >= 0
                want_s = np.where(live, np.take_along_axis(scores, np.maximum(got, 0), 1), 0.0)
                assert np.array_equal(got_s, want_s) and not np.signbit(got_s[got_s == 0]).any(), (topk, sparse, filter_seen)
                if sparse:
                    assert (got[:3] == -1).all()             # the empty row, the zero row, the cancelled row
                if topk > scores.shape[1]:
                    assert (got[:, scores.shape[1]:] == -1).all()
                no_scores, none = hip_ops.spsp_topk(Ld, Bd, topk, filter_seen, sparse)
                assert none is None and np.array_equal(no_scores.cpu().numpy(), got)


def test_two_calls_give_identical_bytes(hip_ops, operands):
    L, B, scores, seen, Ld, Bd = operands[5]
    a = hip_ops.spsp_rows(Ld, Bd).cpu().numpy().tobytes()
    b = hip_ops.spsp_rows(Ld, Bd).cpu().numpy().tobytes()
    assert a == b
    first = [x.cpu().numpy().tobytes() for x in hip_ops.spsp_topk(Ld, Bd, 100, True, True, want_scores=True)]
    second = [x.cpu().numpy().tobytes() for x in hip_ops.spsp_topk(Ld, Bd, 100, True, True, want_scores=True)]
    assert first == second


def test_argument_checks(hip_ops, operands):
    from polara_amd._lib import PolaraHipError
    L, B, scores, seen, Ld, Bd = operands[6]                  # rectangular
    with pytest.raises(PolaraHipError, match='n_inner == n_cols'):
        hip_ops.spsp_topk(Ld, Bd, 10, True, True)
    with pytest.raises(PolaraHipError, match='1024'):
        hip_ops.spsp_topk(Ld, Bd, 1025, False, True)
    with pytest.raises(ValueError, match='columns'):
        hip_ops.spsp_topk(Bd, Bd, 10, False, True)
    with pytest.raises(ValueError, match='rows'):
        hip_ops.spsp_rows(Ld, Bd, rows=(0, L.shape[0] + 1))


# ---- models on the fixtures ----------------------------------------------------------------------------------------------
def _sim_data(g):
    """GoldenData with the item relations of a SIM fixture."""
    data = GoldenData(g)
    n = int(g['train_shape'][1])
    data.item_relations = sps.csr_matrix((g['s_val'], (g['s_row'], g['s_col'])), shape=(n, n))
    data.warm_start = bool(g['warm_start'])
    return data


def _sim_model(g, hip_ops, dense_output=None):
    from polara_amd import SimilarityAggregation
    m = SimilarityAggregation(_sim_data(g), ops=hip_ops)
    m.verbose = False
    m.implicit = bool(g['implicit'])
    m.dense_output = bool(g['dense_output']) if dense_output is None else dense_output
    m.topk = int(g['topk'])
    m.filter_seen = bool(g['filter_seen'])
    return m


def _simcs_model(g, hip_ops):
    from polara_amd import ItemColdStartSimilarityArrayData, SimilarityAggregationItemColdStart
    n_users, n_items = (int(x) for x in g['train_shape'])
    n_cold = int(g['cold_shape'][0])
    idx = g['train_idx']
    data = ItemColdStartSimilarityArrayData(
        (idx[:, 0], idx[:, 1], g['train_val']), (g['hold_user'], g['hold_cold'], g['hold_fdbk']),
        [[0]] * n_items, [[0]] * n_cold, n_users=n_users, n_items=n_items,
        relations_matrices={'itemid': None, 'userid': None}, relations_indices={'itemid': None, 'userid': None},
        cold_relations_matrices={'itemid': sim.cold_similarity(g)})
    m = SimilarityAggregationItemColdStart(data, ops=hip_ops)
    m.verbose = False
    m.implicit = bool(g['implicit'])
    m.topk = int(g['topk'])
    return m


@pytest.mark.parametrize('name', SIM_FIXTURES)
def test_sim_lists_match_the_reference_and_the_restatement(name, hip_ops):
    g = load_golden(name)
    m = _sim_model(g, hip_ops)
    recs = m.recommendations
    scores, cls, lists = sim.sim_lists(g)
    assert recs.shape == g['recs'].shape and recs.dtype == np.int64
    assert ref.tie_aware_mismatches(recs, g['recs'], scores, cls, tol=0.0) == []
    assert np.array_equal(recs, lists)
    again, list_scores = m.recommend_with_scores()
    assert np.array_equal(again, lists)
    want = np.where(lists >= 0, np.take_along_axis(scores, np.maximum(lists, 0), 1), 0.0)
    assert np.array_equal(list_scores, want)
    assert len(m.training_time) == 1
    if name == 'sim_nonsym':
        other = _sim_model(g, hip_ops, dense_output=not bool(g['dense_output']))
        o_scores, o_cls, o_lists = sim.sim_lists(g, dense_output=not bool(g['dense_output']))
        assert np.array_equal(other.recommendations, o_lists)
        assert ref.tie_aware_mismatches(other.recommendations, g['recs_other'], o_scores, o_cls, tol=0.0) == []


@pytest.mark.parametrize('name', SIMCS_FIXTURES)
def test_simcs_lists_match_the_reference_and_the_restatement(name, hip_ops):
    g = load_golden(name)
    m = _simcs_model(g, hip_ops)
    recs = m.recommendations
    scores, cls, lists = sim.simcs_lists(g)
    assert recs.shape == g['recs'].shape and recs.dtype == np.int64
    assert ref.tie_aware_mismatches(recs, g['recs'], scores, cls, tol=0.0) == []
    assert np.array_equal(recs, lists)
    rows = m.slice_recommendations(None, 2, 9)
    assert sps.issparse(rows) and np.array_equal(rows.toarray(), scores[2:9])
    assert len(m.training_time) == 1


def test_sim_lifecycle(hip_ops):
    g = load_golden('sim_sparse')
    m = _sim_model(g, hip_ops)
    recs = m.recommendations
    scores, cls, lists = sim.sim_lists(g)
    assert (recs == -1).any() and len(m.training_time) == 1 and m.build_stats['nnz'] == m.item_similarity_matrix.nnz
    m.topk = 5                                                 # shrinking keeps the cached lists
    assert m.recommendations is recs
    m.topk = int(g['topk'])
    # the host route: score slices, the inherited sparse-aware downvote and selection
    test_data, test_shape, _ = m._get_test_data()
    block, slice_data = m.slice_recommendations(test_data, test_shape, 0, test_shape[0])
    assert sps.issparse(block) and np.array_equal(block.toarray(), scores)
    m.downvote_seen_items(block, slice_data)
    assert np.array_equal(m.get_topk_elements(block), recs)
    m.implicit = True                                          # other test values: new lists, the same model
    assert m._recommendations is None and m._is_ready
    implicit = m.recommendations
    T1 = sim.sim_test_matrix(g, implicit=True)
    s1 = sim.product(T1, sim.similarity(g).T.tocsr())
    assert np.array_equal(implicit, ref.select(s1, sim.seen_mask(T1), m.topk, True, True)) and len(m.training_time) == 1
    m.implicit = False
    m.dense_output = True                                      # the other branch: new lists, the same model
    dense = m.recommendations
    d_scores, _, d_lists = sim.sim_lists(g, dense_output=True)
    assert not (dense == -1).any() and np.array_equal(dense, d_lists) and len(m.training_time) == 1
    block, slice_data = m.slice_recommendations(test_data, test_shape, 0, test_shape[0])
    assert isinstance(block, np.ndarray) and np.array_equal(block, d_scores)
    m.data._notify(m.data.on_change_event)                     # a data change: a new model
    assert m._S is None and not m._is_ready
    m.recommendations
    assert len(m.training_time) == 2
    m.topk = 1025
    with pytest.raises(ValueError, match='1024'):
        m.get_recommendations()


def test_simcs_lifecycle(hip_ops):
    g = load_golden('simcs_sparse')
    m = _simcs_model(g, hip_ops)
    recs = m.recommendations
    assert (recs == -1).any() and len(m.training_time) == 1
    m.implicit = True                                          # the training values change: a new model
    assert not m._is_ready and m._At is None
    ones = m.recommendations
    assert len(m.training_time) == 2 and not np.array_equal(ones, recs)
    gi = dict(g.items())
    gi['implicit'] = np.bool_(True)
    assert np.array_equal(ones, sim.simcs_lists(gi)[2])
    m.dense_output = True
    with pytest.raises(NotImplementedError, match='reference'):
        m.recommendations
