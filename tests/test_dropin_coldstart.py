"""The item cold-start models as drop-ins (no GPU): the reference's `ItemColdStartData` / `ItemColdStartSimilarityData` with a
pandas `item_features` frame feed the reference's own models (through the test-only stand-ins of tests/golden) and ours (on
the CPU double of the device operators) — one data object, the same lists, hit counts and coverage.  Skips where the
reference is not on this machine.  Runs in a child process and compares the metric families that do not go through the
reference's masked division, for the reasons given in tests/test_dropin_hybrid.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'polara')), reason='the reference is not on this machine')


def side_by_side():
    import contextlib
    import io
    import warnings
    warnings.filterwarnings('ignore')
    for p in ('_lightfm_shim', '_sksparse_shim', '_numba_shim'):
        sys.path.insert(0, os.path.join(HERE, 'golden', p))
    sys.path.insert(0, REF)
    import pandas as pd
    from polara.recommender.coldstart.data import ItemColdStartData, ItemColdStartSimilarityData
    from polara.recommender.coldstart import models as refcs
    from polara.lib.similarity import stack_features, cosine_similarity
    from polara_amd import coldstart as ours
    from test_coldstart_host import ColdStartNumpyOps
    rng = np.random.RandomState(5)
    rows = [(u, int(i), float(rng.randint(1, 6))) for u in range(220) for i in rng.choice(110, rng.randint(5, 20), replace=False)]
    df = pd.DataFrame(rows, columns=['userid', 'itemid', 'rating'])
    feat = pd.DataFrame({'genres': [sorted(int(x) for x in rng.choice(30, rng.randint(1, 5), replace=False)) for _ in range(110)]},
                        index=pd.Index(np.arange(110), name='itemid'))
    F, _ = stack_features(feat, normalize=False)
    S = cosine_similarity(F.tocsr().astype(np.float64)).tocsr()
    out = []
    for hybrid, sample in ((False, None), (True, None), (False, 60)):
        if hybrid:
            data = ItemColdStartSimilarityData(df, 'userid', 'itemid', 'rating', seed=3, item_features=feat,
                                               relations_matrices={'itemid': S, 'userid': None},
                                               relations_indices={'itemid': feat.index.values, 'userid': None})
            pairs = [(refcs.HybridSVDItemColdStart, ours.HybridSVDItemColdStart)]
        else:
            data = ItemColdStartData(df, 'userid', 'itemid', 'rating', seed=3, item_features=feat)
            pairs = [(refcs.SVDModelItemColdStart, ours.SVDModelItemColdStart),
                     (refcs.ScaledSVDItemColdStart, ours.ScaledSVDItemColdStart),
                     (refcs.PopularityModelItemColdStart, ours.PopularityModelItemColdStart)]
        data.verbose = False
        if sample:
            data.test_sample = sample
        with contextlib.redirect_stdout(io.StringIO()):
            data.prepare()
        activity = np.bincount(data.training['userid'].values).tolist()
        for ref_cls, our_cls in pairs:
            pair = []
            for m in (ref_cls(data), our_cls(data, ops=ColdStartNumpyOps())):
                m.verbose = False
                if hasattr(m, 'rank'):
                    m.rank = 8
                with contextlib.redirect_stdout(io.StringIO()):
                    m.build()
                    recs = np.asarray(m.get_recommendations())
                    scores = {type(x).__name__: x for x in m.evaluate(['hits', 'experience'])}
                    recs5 = None
                    if hasattr(m, 'rank'):
                        m.rank = 5
                        recs5 = np.asarray(m.get_recommendations()).tolist()
                pair.append(dict(method=m.method, recs=recs.tolist(), recs5=recs5, builds=len(m.training_time),
                                 hits=[int(x) if x is not None else None for x in scores['Hits']],
                                 coverage=float(scores['Experience'].coverage), key=m._prediction_key,
                                 target=m._prediction_target, filter_seen=bool(m.filter_seen)))
            out.append(dict(pair=pair, activity=activity, sample=sample))
    return out


def test_reference_data_objects_drive_both_models():
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.dirname(HERE), HERE] + ([env['PYTHONPATH']] if env.get('PYTHONPATH') else []))
    flags = ['-s'] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + [os.path.abspath(__file__)], cwd=HERE, env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    results = json.loads(r.stdout.strip().splitlines()[-1])
    assert [x['pair'][0]['method'] for x in results] == ['PureSVD(cs)', 'PureSVD(cs)-s', 'MP(cs)', 'HybridSVD(cs)', 'PureSVD(cs)',
                                                         'PureSVD(cs)-s', 'MP(cs)']
    for x in results:
        ref, ours = x['pair']
        for k in ('method', 'key', 'target', 'filter_seen', 'builds'):
            assert ref[k] == ours[k], (ref['method'], k)
        a, b = np.asarray(ours['recs']), np.asarray(ref['recs'])
        if ref['method'] == 'MP(cs)':
            # the reference's sort leaves users of equal activity in no defined order: the activity of the listed users
            act = np.asarray(x['activity'])
            assert a.shape == b.shape and np.array_equal(act[a], act[b])
            continue
        assert np.array_equal(a, b) and np.array_equal(np.asarray(ours['recs5']), np.asarray(ref['recs5']))
        assert ours['hits'] == ref['hits'] and ours['coverage'] == ref['coverage']


if __name__ == '__main__':
    print(json.dumps(side_by_side()))
