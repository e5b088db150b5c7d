"""The LightFM models as drop-ins (no GPU): the reference's `RecommenderData` / `ItemColdStartData` with a pandas
`item_features` frame feed `LightFMWrapper` / `LightFMItemColdStart` on the CPU double of the device operators.  The reference's
own wrapper cannot run (the `lightfm` package is not a dependency), so the build is compared with the restated fit
(tests/lightfm_reference.py) on the same training matrix and the one-hot matrix `stack_features` gives for the re-indexed frame,
and the lists with `argsort` of the restated scores.  Skips where the reference is not on this machine.  Runs in a child
process, like tests/test_dropin_lce.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'polara')), reason='the reference is not on this machine')

SETTINGS = dict(rank=5, learning_rate=0.05, max_sampled=6, num_epochs=3, seed=11, blocks=3)


def side_by_side():
    import contextlib
    import io
    import warnings
    warnings.filterwarnings('ignore')
    for p in ('_lightfm_shim', '_sksparse_shim', '_numba_shim'):
        sys.path.insert(0, os.path.join(HERE, 'golden', p))
    sys.path.insert(0, REF)
    import pandas as pd
    from polara.recommender.data import RecommenderData
    from polara.recommender.coldstart.data import ItemColdStartData
    from polara_amd import warp
    from polara_amd.coldstart import stack_features
    import lightfm_reference as ref
    rng = np.random.RandomState(5)
    rows = [(u, int(i), float(rng.randint(1, 6))) for u in range(120) for i in rng.choice(70, rng.randint(5, 15), replace=False)]
    df = pd.DataFrame(rows, columns=['userid', 'itemid', 'rating'])
    feat = pd.DataFrame({'genres': [sorted(int(x) for x in rng.choice(12, rng.randint(1, 4), replace=False)) for _ in range(70)]},
                        index=pd.Index(np.arange(70), name='itemid'))
    out = []
    for cold in (False, True):
        if cold:
            data = ItemColdStartData(df, 'userid', 'itemid', 'rating', seed=3, item_features=feat)
        else:
            data = RecommenderData(df, 'userid', 'itemid', 'rating', seed=3)
            data.warm_start = False
            data.holdout_size = 3
        data.verbose = False
        with contextlib.redirect_stdout(io.StringIO()):
            data.prepare()
        m = (warp.LightFMItemColdStart if cold else warp.LightFMWrapper)(data, item_features=feat, ops=ref.numpy_ops())
        m.verbose = False
        m.rank, m.learning_rate, m.max_sampled, m.seed = (SETTINGS[k] for k in ('rank', 'learning_rate', 'max_sampled', 'seed'))
        m.fit_params, m.blocks, m.topk = dict(epochs=SETTINGS['num_epochs']), SETTINGS['blocks'], 5
        with contextlib.redirect_stdout(io.StringIO()):
            m.build()
            recs = np.asarray(m.get_recommendations())
            scores = m.evaluate()
        dense = (m.get_training_matrix().toarray() != 0).astype(np.int8)
        index = data.index.itemid
        index = getattr(index, 'training', index)
        one_hot, labels = stack_features(feat.reindex(index.old.values, fill_value=[]))
        want = ref.fit(dense, one_hot=one_hot.toarray(), **SETTINGS)
        itemid = data.fields.itemid
        same = lambda a, b: bool(a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64)))
        equal = dict(P=same(m.factors[data.fields.userid], want['P']), Q=same(m.factors[itemid], want['Q']),
                     E=same(m.factors[f'{itemid}_identity'], want['E']), L=same(m.factors[f'{itemid}_features'], want['L']),
                     history=list(m.warp_history) == want['history'], labels=m.item_features_labels == labels)
        if cold:
            cold_frame = feat.reindex(data.index.itemid.cold_start.old.values, fill_value=[])
            cold_hot = stack_features(cold_frame, labels=labels)[0].toarray()
            restated = ref.cold_queries(cold_hot, want['L']) @ want['P'].T
            lists = ref.top_lists(restated, m.topk, np.zeros_like(restated))
        else:
            test_users = np.asarray(m._get_test_data()[2])
            restated = (want['P'] @ want['Q'].T)[test_users]
            lists = ref.top_lists(restated, m.topk, dense[test_users])
        ranked = -np.sort(-restated, axis=1)
        out.append(dict(method=m.method, cold=cold, equal=equal, recs=recs.tolist(), lists=lists.tolist(), shape=list(recs.shape),
                        n_rows=int(restated.shape[0]), key=m._prediction_key if cold else None, n_scores=len(scores),
                        ties=int((ranked[:, m.topk - 1] == ranked[:, m.topk]).sum()) if cold else 0))
    return out


def test_reference_data_objects_drive_both_models():
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.dirname(HERE), HERE] + ([env['PYTHONPATH']] if env.get('PYTHONPATH') else []))
    flags = ['-s'] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + [os.path.abspath(__file__)], cwd=HERE, env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    results = json.loads(r.stdout.strip().splitlines()[-1])
    assert [x['method'] for x in results] == ['LightFM', 'LightFM(cs)']
    for x in results:
        assert all(x['equal'].values()), x['equal']
        assert x['shape'] == [x['n_rows'], 5] and x['n_scores'] > 0 and x['ties'] == 0
        assert np.array_equal(np.asarray(x['recs']), np.asarray(x['lists']))
    assert results[1]['key'] == 'itemid_cold'


if __name__ == '__main__':
    print(json.dumps(side_by_side()))
