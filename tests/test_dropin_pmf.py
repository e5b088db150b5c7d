"""ProbabilisticMF as a drop-in (no GPU): the reference's `RecommenderData` feeds the reference's own `ProbabilisticMF`
(through the test-only stand-ins of tests/golden) and ours (on the CPU double of the device operators, blocks = 1: the
reference's own order of the samples) — one data object, the reference's function objects as `adjust_gradient`, the same
lists and evaluate() numbers.  Skips where the reference is not on this machine.  Runs in a child process, like
tests/test_dropin_lce.py."""
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
    from polara.lib import optimize
    from polara.recommender.data import RecommenderData
    from polara.recommender.models import ProbabilisticMF as RefPMF
    from polara_amd import pmf as ours
    from pmf_reference import PMFNumpyOps
    from test_coldstart_host import EVAL_KEYS
    rng = np.random.RandomState(5)
    rows = [(u, int(i), float(rng.randint(1, 6))) for u in range(220) for i in rng.choice(110, rng.randint(5, 20), replace=False)]
    df = pd.DataFrame(rows, columns=['userid', 'itemid', 'rating'])
    data = RecommenderData(df, 'userid', 'itemid', 'rating', seed=3)
    data.warm_start = False
    data.holdout_size = 3
    data.verbose = False
    with contextlib.redirect_stdout(io.StringIO()):
        data.prepare()
    out = []
    # (adjust_gradient, learn_rate, epochs): the adaptive runs are short — at this rate they amplify a last-bit difference by
    # an order of magnitude per epoch (tests/golden/make_golden_pmf.py)
    for adjust, rate, epochs in ((None, 0.005, 25), (optimize.adagrad, 0.05, 3), (optimize.rmsprop, 0.05, 3)):
        pair = []
        for is_ref in (True, False):
            m = RefPMF(data, seed=11) if is_ref else ours.ProbabilisticMF(data, seed=11, ops=PMFNumpyOps())
            m.verbose = False
            m.rank, m.learn_rate, m.num_epochs = 8, rate, epochs
            if not is_ref:
                m.blocks = 1
            with contextlib.redirect_stdout(io.StringIO()):
                m.build(**({'adjust_gradient': adjust} if adjust else {}))
                recs = np.asarray(m.get_recommendations())
                scores = {type(x).__name__: x for x in m.evaluate('all')}
            numbers = {}
            for key in EVAL_KEYS:
                _, family, field = key.split('_', 2)
                numbers[key] = float(getattr(scores[family], field))
            pair.append(dict(method=m.method, recs=recs.tolist(), numbers=numbers, key=m._prediction_key, target=m._prediction_target,
                             filter_seen=bool(m.filter_seen), builds=len(m.training_time), epochs=len(m.rmse_history),
                             times=len(m.iterations_time), rmse=[float(x) for x in m.rmse_history],
                             shapes={k: list(np.asarray(v).shape) for k, v in m.factors.items()}))
        out.append(dict(pair=pair, adjust=getattr(adjust, '__name__', None)))
    return out


def test_reference_data_object_drives_both_models():
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.dirname(HERE), HERE] + ([env['PYTHONPATH']] if env.get('PYTHONPATH') else []))
    flags = ['-s'] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + [os.path.abspath(__file__)], cwd=HERE, env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    results = json.loads(r.stdout.strip().splitlines()[-1])
    assert [x['adjust'] for x in results] == [None, 'adagrad', 'rmsprop']
    for x in results:
        ref, ours = x['pair']
        for k in ('method', 'key', 'target', 'filter_seen', 'builds', 'epochs', 'times', 'shapes'):
            assert ref[k] == ours[k], (x['adjust'], k)
        assert ref['method'] == 'PMF' and set(ours['shapes']) == {'userid', 'itemid'}
        assert np.allclose(ours['rmse'], ref['rmse'], rtol=1e-12, atol=0)
        assert np.array_equal(np.asarray(ours['recs']), np.asarray(ref['recs']))
        for key, value in ref['numbers'].items():
            assert np.isclose(ours['numbers'][key], value, rtol=1e-12, atol=0), key


if __name__ == '__main__':
    print(json.dumps(side_by_side()))
