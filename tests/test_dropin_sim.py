"""SimilarityAggregation and SIM(cs) as drop-ins (no GPU): the reference's `SimilarityDataModel` and
`ItemColdStartSimilarityData` feed the reference's own models (through the test-only stand-ins of tests/golden) and ours (on
a CPU double of the two device operators: SciPy's product and the selection of tests/i2i_reference.py) — one data object,
the same lists up to ties.  Skips where the reference is not on this machine.  Runs in a child process, like
tests/test_dropin_coldstart.py.

The reference's sparse `downvote_seen_items` has no effect (its last line rebinds a local name); SIM is
therefore compared with `filter_seen=False` in the sparse branch and with `filter_seen=True` in the dense one."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'polara')), reason='the reference is not on this machine')


def sim_numpy_ops():
    """The CPU double of the operators the two models use."""
    import scipy.sparse as sps
    import torch
    import i2i_reference as ref
    import sim_reference as sim
    from numpy_ops import NpCSR, NumpyOps

    class Csr(NpCSR):
        """NpCSR that keeps the stored order of its rows and carries `values` (what the models rewrite under `implicit`)."""

        def __init__(self, indptr, indices, values, shape):
            super().__init__(indptr, indices, values, shape)
            self.values = torch.from_numpy(np.asarray(values, dtype=np.float64).copy())

        def with_columns(self, indices, values):
            return Csr(self.indptr.numpy(), np.asarray(indices), np.asarray(values), self.shape)

        @property
        def T(self):
            t = self.m.T.tocsr()
            t.sort_indices()
            return Csr(t.indptr, t.indices, t.data, t.shape)

    class SimNumpyOps(NumpyOps):
        def csr(self, indptr, indices, values, shape, split=None):
            return Csr(indptr, indices, values, shape)

        def csr_from_coo(self, rows, cols, vals, shape, split=None):
            a = super().csr_from_coo(rows, cols, vals, shape)
            return Csr(a.m.indptr, a.m.indices, a.m.data, shape)

        def spsp_rows(self, L, B, rows=None):
            lo, hi = (0, L.shape[0]) if rows is None else rows
            return torch.from_numpy(sim.product(L.m[lo:hi], B.m))

        def spsp_topk(self, L, B, topk, filter_seen, sparse, want_scores=False):
            scores = sim.product(L.m, B.m)
            seen = sim.seen_mask(L.m) if filter_seen else np.zeros(scores.shape, dtype=bool)
            lists = ref.select(scores, seen, int(topk), filter_seen, sparse)
            s = np.where(lists >= 0, np.take_along_axis(scores, np.maximum(lists, 0), 1), 0.0)
            return torch.from_numpy(lists), (torch.from_numpy(s) if want_scores else None)

    return SimNumpyOps()


def side_by_side():
    import contextlib
    import io
    import warnings
    warnings.filterwarnings('ignore')
    for p in ('_lightfm_shim', '_sksparse_shim', '_numba_shim'):
        sys.path.insert(0, os.path.join(HERE, 'golden', p))
    sys.path.insert(0, REF)
    import pandas as pd
    import scipy.sparse as sps
    from polara.recommender.hybrid.data import SimilarityDataModel
    from polara.recommender.hybrid.models import SimilarityAggregation as RefSim
    from polara.recommender.coldstart.data import ItemColdStartSimilarityData
    from polara.recommender.coldstart.models import SimilarityAggregationItemColdStart as RefSimCS
    from polara.lib.similarity import stack_features, cosine_similarity
    from polara.lib.sparse import sparse_dot
    from polara_amd import SimilarityAggregation, SimilarityAggregationItemColdStart
    rng = np.random.RandomState(9)
    n_users, n_items, n_labels = 260, 900, 120
    rows = [(u, int(i), float(rng.randint(1, 6))) for u in range(n_users) for i in rng.choice(n_items, rng.randint(4, 12), replace=False)]
    df = pd.DataFrame(rows, columns=['userid', 'itemid', 'rating'])
    feat = pd.DataFrame({'genres': [sorted(int(x) for x in rng.choice(n_labels, rng.randint(1, 4), replace=False))
                                    for _ in range(n_items)]}, index=pd.Index(np.arange(n_items), name='itemid'))
    F, _ = stack_features(feat, normalize=False)
    S = cosine_similarity(F.tocsr().astype(np.float64)).tocsr()
    out = []

    def run(m, settings):
        m.verbose = False
        for k, v in settings.items():
            setattr(m, k, v)
        with contextlib.redirect_stdout(io.StringIO()):
            m.build()
            return np.asarray(m.get_recommendations())

    data = SimilarityDataModel(df, 'userid', 'itemid', 'rating', seed=0, relations_matrices={'itemid': S, 'userid': None},
                               relations_indices={'itemid': np.arange(n_items), 'userid': None})
    data.verbose = False
    data.warm_start = False
    data.holdout_size = 1
    data.test_ratio, data.test_fold = 0.5, 2
    with contextlib.redirect_stdout(io.StringIO()):
        data.prepare()
    for settings in (dict(topk=10, filter_seen=False, dense_output=False, implicit=False),
                     dict(topk=10, filter_seen=False, dense_output=False, implicit=True),
                     dict(topk=10, filter_seen=True, dense_output=True, implicit=False)):
        ref_m, our_m = RefSim(data), SimilarityAggregation(data, ops=sim_numpy_ops())
        a, b = run(ref_m, settings), run(our_m, settings)
        test_data, shape, _ = our_m._get_test_data()
        scores, _ = our_m.slice_recommendations(test_data, shape, 0, shape[0])
        scores = np.asarray(scores.toarray() if sps.issparse(scores) else scores)
        seen = np.zeros(scores.shape, dtype=bool)
        seen[test_data[0], test_data[1]] = settings['filter_seen']
        out.append(dict(method=[ref_m.method, our_m.method], settings=settings, ref=a.tolist(), ours=b.tolist(),
                        scores=scores.tolist(), seen=seen.tolist(), builds=[len(ref_m.training_time), len(our_m.training_time)]))

    cs = ItemColdStartSimilarityData(df, 'userid', 'itemid', 'rating', seed=3, item_features=feat,
                                     relations_matrices={'itemid': S, 'userid': None},
                                     relations_indices={'itemid': feat.index.values, 'userid': None})
    cs.verbose = False
    with contextlib.redirect_stdout(io.StringIO()):
        cs.prepare()
    for settings in (dict(topk=10, implicit=False), dict(topk=10, implicit=True)):
        ref_m, our_m = RefSimCS(cs), SimilarityAggregationItemColdStart(cs, ops=sim_numpy_ops())
        a, b = run(ref_m, settings), run(our_m, settings)
        A = ref_m.get_training_matrix()
        if settings['implicit']:
            A.data = np.ones_like(A.data)
        scores = sparse_dot(cs.cold_items_similarity, A, False, True)
        scores = np.asarray(scores.toarray() if sps.issparse(scores) else scores)
        out.append(dict(method=[ref_m.method, our_m.method], settings=dict(settings, filter_seen=False, dense_output=False),
                        ref=a.tolist(), ours=b.tolist(), scores=scores.tolist(), seen=np.zeros(scores.shape, dtype=bool).tolist(),
                        key=[ref_m._prediction_key, our_m._prediction_key], target=[ref_m._prediction_target, our_m._prediction_target]))
    return out


def test_reference_data_objects_drive_both_models():
    import i2i_reference as ref
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.dirname(HERE), HERE] + ([env['PYTHONPATH']] if env.get('PYTHONPATH') else []))
    flags = ['-s'] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + [os.path.abspath(__file__)], cwd=HERE, env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    results = json.loads(r.stdout.strip().splitlines()[-1])
    assert [x['method'] for x in results] == [['SIM', 'SIM']] * 3 + [['SIM(cs)', 'SIM(cs)']] * 2
    for x in results:
        s = x['settings']
        ours, theirs = np.asarray(x['ours']), np.asarray(x['ref'])
        scores, seen = np.asarray(x['scores']), np.asarray(x['seen'])
        assert ours.shape == theirs.shape and ours.shape[0] >= 20
        cls = ref.classes(scores, seen, s['filter_seen'], not s['dense_output'])
        assert ref.tie_aware_mismatches(ours, theirs, scores, cls, tol=0.0) == [], (x['method'], s)
        if 'key' in x:
            assert x['key'][0] == x['key'][1] and x['target'][0] == x['target'][1]


if __name__ == '__main__':
    print(json.dumps(side_by_side()))
