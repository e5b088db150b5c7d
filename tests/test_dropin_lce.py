"""The LCE models as drop-ins (no GPU): the reference's `RecommenderData` / `ItemColdStartData` with a pandas `item_features`
frame feed the reference's own `LCEModel` / `LCEModelItemColdStart` (through the test-only stand-ins of tests/golden) and ours
(on the CPU double of the device operators) — one data object with the item column called `item` (the only name under which
the reference's LCE(cs) finds its own factors), the graph taken from the reference, the same lists and evaluate() numbers.
Skips where the reference is not on this machine.  Runs in a child process, like tests/test_dropin_coldstart.py."""
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
    from polara.recommender.data import RecommenderData
    from polara.recommender.coldstart.data import ItemColdStartData
    from polara.recommender.coldstart.models import LCEModelItemColdStart as RefCold
    from polara.recommender.hybrid.models import LCEModel as RefLCE
    from polara_amd import lce as ours
    from lce_reference import LCENumpyOps
    from test_coldstart_host import EVAL_KEYS
    rng = np.random.RandomState(5)
    rows = [(u, int(i), float(rng.randint(1, 6))) for u in range(220) for i in rng.choice(110, rng.randint(5, 20), replace=False)]
    df = pd.DataFrame(rows, columns=['userid', 'item', 'rating'])
    feat = pd.DataFrame({'genres': [sorted(int(x) for x in rng.choice(30, rng.randint(1, 5), replace=False)) for _ in range(110)]},
                        index=pd.Index(np.arange(110), name='item'))
    out = []
    for cold, sample in ((False, None), (True, None), (True, 60)):
        if cold:
            data = ItemColdStartData(df, 'userid', 'item', 'rating', seed=3, item_features=feat)
        else:
            data = RecommenderData(df, 'userid', 'item', 'rating', seed=3)
            data.warm_start = False
            data.holdout_size = 3
        data.verbose = False
        if sample:
            data.test_sample = sample
        with contextlib.redirect_stdout(io.StringIO()):
            data.prepare()
        graphs = []
        build_graph = RefLCE.build_item_graph

        def keep_graph(model, item_features, n_neighbors):
            graphs.append(build_graph(model, item_features, n_neighbors))
            return graphs[-1]
        pair = []
        for is_ref in (True, False):
            if is_ref:
                m = (RefCold if cold else RefLCE)(data, item_features=feat)
                RefLCE.build_item_graph = keep_graph
            else:
                m = (ours.LCEModelItemColdStart if cold else ours.LCEModel)(data, item_features=feat, ops=LCENumpyOps())
                m.item_graph = graphs[0]
            m.verbose = False
            m.rank, m.seed = 8, 11
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    m.build()
                    recs = np.asarray(m.get_recommendations())
                    scores = {type(x).__name__: x for x in m.evaluate('all')}
            finally:
                RefLCE.build_item_graph = build_graph
            numbers = {}
            for key in EVAL_KEYS:
                _, family, field = key.split('_', 2)
                numbers[key] = float(getattr(scores[family], field))
            itemid = data.fields.itemid
            pair.append(dict(method=m.method, recs=recs.tolist(), numbers=numbers, key=m._prediction_key, target=m._prediction_target,
                             filter_seen=bool(m.filter_seen), builds=len(m.training_time),
                             shapes={k: list(np.asarray(v).shape) for k, v in m.factors.items()}, itemid=itemid))
        out.append(dict(pair=pair, cold=cold, sample=sample))
    return out


def test_reference_data_objects_drive_both_models():
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.dirname(HERE), HERE] + ([env['PYTHONPATH']] if env.get('PYTHONPATH') else []))
    flags = ['-s'] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + [os.path.abspath(__file__)], cwd=HERE, env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    results = json.loads(r.stdout.strip().splitlines()[-1])
    assert [x['pair'][0]['method'] for x in results] == ['LCE', 'LCE(cs)', 'LCE(cs)']
    for x in results:
        ref, ours = x['pair']
        for k in ('method', 'key', 'target', 'filter_seen', 'builds', 'shapes', 'itemid'):
            assert ref[k] == ours[k], (ref['method'], k)
        assert ref['itemid'] == 'item' and set(ours['shapes']) == {'userid', 'item', 'item_features'}
        assert np.array_equal(np.asarray(ours['recs']), np.asarray(ref['recs']))
        for key, value in ref['numbers'].items():
            assert np.isclose(ours['numbers'][key], value, rtol=1e-12, atol=0), key


if __name__ == '__main__':
    print(json.dumps(side_by_side()))
