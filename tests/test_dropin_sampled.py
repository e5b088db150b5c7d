"""The sampled-evaluation models as drop-ins (no GPU): the reference's `RecommenderData` under its own
`RandomSampleEvaluationMixin` feeds the reference's `SVDModel` under `RandomSampleEvaluationSVDMixin` (through the test-only
stand-ins of tests/golden) and our `SVDModelSampled` (on a CPU double of the operators: tests/numpy_ops.py plus the
restatements of tests/sampled_reference.py for the two new ones) — one data object.  Compared: the lists, the three
`compute_*` arrays (both fed the reference's factors: bit-equal, except the sampled one, whose streams differ by design and
which is held to its definition instead) and the metric tuples.  Skips where the reference is not on this machine.  Runs in a
child process, like tests/test_dropin_sim.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'polara')), reason='the reference is not on this machine')


def sampled_numpy_ops():
    """The CPU double of the operators the sampled models use."""
    import torch
    import sampled_reference as ref
    from numpy_ops import NumpyOps

    class SampledNumpyOps(NumpyOps):
        def candidates_topk(self, P, V, cand, topk, want_scores=False):
            lists, scores = ref.candidates_topk(P.numpy(), V.numpy(), cand.numpy(), topk)
            return torch.from_numpy(lists), (torch.from_numpy(scores) if want_scores else None)

        def sample_unseen(self, T, H, n, seeds):
            t, h = T.m, (None if H is None else H.m)
            t.sort_indices()
            return torch.from_numpy(ref.sample_unseen(t.indptr, t.indices, None if h is None else h.indptr,
                                                      None if h is None else h.indices, T.shape[1], n, seeds))

    return SampledNumpyOps()


def side_by_side():
    import contextlib
    import io
    import warnings
    warnings.filterwarnings('ignore')
    for p in ('_lightfm_shim', '_sksparse_shim', '_numba_shim'):
        sys.path.insert(0, os.path.join(HERE, 'golden', p))
    sys.path.insert(0, REF)
    import pandas as pd
    from polara.recommender.data import RecommenderData, RandomSampleEvaluationMixin as RefDataMixin
    from polara.recommender.models import SVDModel as RefSVD, RandomSampleEvaluationSVDMixin as RefMixin
    from polara_amd import SVDModelSampled

    class D(RefDataMixin, RecommenderData):
        pass

    class RefSampled(RefMixin, RefSVD):
        pass

    def quiet(fn, *a):
        with contextlib.redirect_stdout(io.StringIO()):
            return fn(*a)

    out = []
    for holdout_size, warm_start, seed in ((1, True, 3), (2, False, 4)):
        rng = np.random.RandomState(seed)
        n_users, n_items, n_unseen = 160, 300, 25
        rows = [(u, int(i), float(rng.randint(1, 6))) for u in range(n_users)
                for i in rng.choice(n_items, rng.randint(10, 30), replace=False)]
        data = D(pd.DataFrame(rows, columns=['userid', 'itemid', 'rating']), 'userid', 'itemid', 'rating', seed=seed)
        data.verbose = False
        data.warm_start, data.holdout_size = warm_start, holdout_size
        data.test_ratio, data.test_fold = 0.5, 2
        quiet(data.prepare)
        ref_m, our_m = RefSampled(data), SVDModelSampled(data, ops=sampled_numpy_ops())
        for m in (ref_m, our_m):
            m.verbose = False
            m.rank, m.topk = 8, 10
        (tu, ti, tf), tshape, _ = ref_m._get_test_data()
        hold = data.test.holdout
        test_users = hold['userid'].drop_duplicates().values
        hold_row = pd.factorize(hold['userid'].values, sort=False)[0]
        unseen = np.stack([rng.choice(np.setdiff1d(np.arange(tshape[1]), np.union1d(ti[tu == r], hold['itemid'].values[hold_row == r])),
                                      n_unseen, replace=False) for r in range(tshape[0])])
        data.set_unseen_interactions(pd.Series(list(unseen), index=pd.Index(test_users, name='userid')), reindex=False)
        np.random.seed(seed)
        quiet(ref_m.build)
        quiet(our_m.build)
        a, b = np.asarray(ref_m.get_recommendations()), np.asarray(our_m.get_recommendations())
        V = ref_m.factors['itemid']
        test_matrix, _ = ref_m.get_test_matrix()
        U = test_matrix.dot(V)
        ref_scores = np.concatenate((ref_m.compute_holdout_scores(U, V), ref_m.compute_random_item_scores(U, V)), axis=1)
        our_scores = np.concatenate((our_m.compute_holdout_scores(U, V), our_m.compute_random_item_scores(U, V)), axis=1)
        metrics = {k: ([None if x is None else float(x) for x in ref_m.evaluate(k)], [None if x is None else float(x) for x in our_m.evaluate(k)])
                   for k in ('relevance', 'ranking', 'hits')}
        # the sampled path: our stream, held to its definition
        gen = our_m.compute_random_item_scores_gen(U, V, test_matrix, n_unseen)
        data.unseen_interactions = None
        our_m._recommendations = None
        _, gen_scores, gen_items = our_m.recommend_with_scores()
        gen_lists = np.asarray(our_m.get_recommendations())
        excluded_hit = any(set(gen_items[r].tolist()[holdout_size:]) & (set(ti[tu == r].tolist()) | set(hold['itemid'].values[hold_row == r].tolist()))
                           for r in range(tshape[0]))
        data.unseen_items_num = None
        our_m._recommendations = None
        try:
            our_m.get_recommendations()
            unspecified = None
        except ValueError as exc:
            unspecified = str(exc)
        out.append(dict(ref=a.tolist(), ours=b.tolist(), ref_scores=ref_scores.tolist(), our_scores=our_scores.tolist(),
                        metrics=metrics, target=[ref_m._prediction_target, our_m._prediction_target], topk=10,
                        gen_shape=list(gen.shape), gen_scores=gen_scores.tolist(), gen_lists=gen_lists.tolist(),
                        gen_items_distinct=all(len(set(r[holdout_size:])) == n_unseen for r in gen_items.tolist()),
                        gen_hold_first=bool(np.array_equal(gen_items[:, :holdout_size], hold['itemid'].values.reshape(-1, holdout_size))),
                        excluded_hit=bool(excluded_hit), unspecified=unspecified, holdout_size=holdout_size,
                        builds=[len(ref_m.training_time), len(our_m.training_time)]))
    return out


def test_reference_data_object_drives_both_models():
    import sampled_reference as ref
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.dirname(HERE), HERE] + ([env['PYTHONPATH']] if env.get('PYTHONPATH') else []))
    flags = ['-s'] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + [os.path.abspath(__file__)], cwd=HERE, env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    results = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(results) == 2
    for x in results:
        assert x['target'] == ['x_itemid', 'x_itemid'] and x['builds'] == [1, 1]
        ours, theirs = np.asarray(x['ours']), np.asarray(x['ref'])
        ref_scores, our_scores = np.asarray(x['ref_scores']), np.asarray(x['our_scores'])
        assert ours.shape == theirs.shape and ours.shape[0] >= 50
        assert np.array_equal(ref_scores, our_scores)                    # the same factors in: bit-equal
        # the two builds give factors that agree to rounding; every row's top-(k+1) scores are apart (the seeds are fixed: should
        # one ever fail this, choose another the way tests/golden/make_golden_sampled.py does), so every row is compared
        top = -np.sort(-ref_scores, axis=1)[:, :x['topk'] + 1]
        assert ((top[:, :-1] - top[:, 1:]).min(axis=1) > 1e-6 * np.abs(ref_scores).max()).all()
        assert np.array_equal(ours, theirs)
        for kind, (a, b) in x['metrics'].items():
            assert len(a) == len(b) and len(a) >= 1, kind
            for p, q in zip(a, b):
                assert (p is None or np.isnan(p)) if (q is None or np.isnan(q)) else p == pytest.approx(q, rel=1e-12), kind
        # the sampled path
        assert x['gen_shape'] == [ours.shape[0], 25] and x['gen_items_distinct'] and x['gen_hold_first'] and not x['excluded_hit']
        assert np.array_equal(np.asarray(x['gen_lists']), ref.select(np.asarray(x['gen_scores']), x['topk']))
        assert x['unspecified'] == 'Number of items to sample is unspecified.'


if __name__ == '__main__':
    print(json.dumps(side_by_side()))
