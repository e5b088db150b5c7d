"""HybridSVD as a drop-in (no GPU): the reference's `SimilarityDataModel` feeds the reference's own `HybridSVD` (through
the test-only scikit-sparse stand-in of tests/golden/_sksparse_shim) and ours (on the CPU double of the device
operators) — one data object, the same lists and metrics.  Skips where the reference is not on this machine.

The side-by-side runs in a child process.  The reference's relevance and ranking metrics divide with
`np.divide(a, b, where=mask)` and no `out=` (polara/recommender/evaluation.py:18-20), so the entries outside the mask are
whatever the allocator hands back: their values depend on the allocation history of the process.  Running the
reference's evaluation here would change that history for every later test that compares those metrics
(tests/test_dropin_polara.py); in a child process nothing is left behind.  For the same reason the comparison below
takes the metrics that do not go through that division: the hit counts and the coverage."""
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
    """(lists, hits, coverage) of the reference's HybridSVD and ours on one SimilarityDataModel, as plain lists."""
    import contextlib
    import io
    import warnings
    warnings.filterwarnings('ignore')
    for p in (os.path.join(HERE, 'golden', '_sksparse_shim'), os.path.join(HERE, 'golden', '_numba_shim'), REF):
        sys.path.insert(0, p)
    import pandas as pd
    import scipy.sparse as sps
    from polara.recommender.hybrid.data import SimilarityDataModel
    from polara.recommender.hybrid.models import HybridSVD as RefHybrid
    from polara_amd.models import HybridSVD
    from test_hybrid_host import HybridNumpyOps
    rng = np.random.RandomState(21)
    rows = [(u, int(i), float(rng.randint(1, 6))) for u in range(200) for i in rng.choice(90, rng.randint(4, 16), replace=False)]
    df = pd.DataFrame(rows, columns=['userid', 'itemid', 'rating'])
    F = (sps.csr_matrix((rng.rand(90, 30) < 0.1).astype(float))
         + sps.csr_matrix((np.ones(90), (np.arange(90), rng.randint(0, 30, 90))), shape=(90, 30)))
    F.data[:] = 1.0
    Fn = sps.diags(1 / np.sqrt(np.asarray(F.sum(1)).ravel())) @ F
    S = (Fn @ Fn.T).tocsr()
    data = SimilarityDataModel(df, 'userid', 'itemid', 'rating', seed=0, relations_matrices={'itemid': S, 'userid': None},
                               relations_indices={'itemid': np.arange(90), 'userid': None})
    data.verbose = False
    data.holdout_size = 2
    with contextlib.redirect_stdout(io.StringIO()):
        data.prepare()
    out = []
    for m in (RefHybrid(data), HybridSVD(data, ops=HybridNumpyOps())):
        m.verbose = False
        m.rank = 8
        with contextlib.redirect_stdout(io.StringIO()):
            m.build()
            recs = np.asarray(m.get_recommendations())
            scores = {type(x).__name__: x for x in m.evaluate(['hits', 'experience'])}
        out.append(dict(method=m.method, recs=recs.tolist(),
                        hits=[int(x) if x is not None else None for x in scores['Hits']],
                        coverage=float(scores['Experience'].coverage)))
    return out


def test_reference_data_object_drives_both_models():
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.dirname(HERE), HERE] + ([env['PYTHONPATH']] if env.get('PYTHONPATH') else []))
    flags = ['-s'] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + [os.path.abspath(__file__)], cwd=HERE, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    ref, ours = json.loads(r.stdout.strip().splitlines()[-1])
    assert ref['method'] == ours['method'] == 'HybridSVD'
    assert np.array_equal(np.asarray(ours['recs']), np.asarray(ref['recs']))
    assert ours['hits'] == ref['hits'] and ours['coverage'] == ref['coverage']


if __name__ == '__main__':
    print(json.dumps(side_by_side()))
