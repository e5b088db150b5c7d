"""Records what the REFERENCE's evaluation code returns on the inputs of two tests of tests/test_dropin_polara.py, so that
they run wherever the reference is absent: tests/golden/dropin_metrics.npz.

  * test_native_metrics_equal_the_reference_evaluate: for each data configuration, the lists of the reference's
    `SVDModel` (rank 6, top-12) on Polara's own `RecommenderData`, the holdout they are scored against, and the numbers
    of the reference's `evaluate('all')` for every (topk, switch_positive) the test visits;
  * test_zero_feedback_holdout_entries_count_like_the_reference: the reference's hit counts, MAP, ARHR, HR and MRR on the
    seeded lists and holdout (with feedback-0 entries) the test draws itself.

usage:  python tests/golden/make_dropin_metrics.py <path of a checkout of the reference (the directory holding polara/)>
"""
import contextlib
import io
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.abspath(sys.argv[1])
sys.path.insert(0, os.path.join(HERE, '_numba_shim'))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
warnings.filterwarnings('ignore')

import numpy as np
import pandas as pd

import polara
from polara.recommender import evaluation as rev

import test_dropin_polara as T

NAN = float('nan')


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def hits_array(h):
    return np.array([NAN if x is None else float(x) for x in h])


def main():
    out = {}
    for cid, cfg in zip(T.METRIC_CFG_IDS, T.METRIC_CFGS):
        data = T.make_data(polara, **cfg)
        ref_m = polara.SVDModel(data)
        ref_m.verbose = False
        ref_m.rank, ref_m.topk = 6, 12
        np.random.seed(0)
        quiet(ref_m.build)
        recs = ref_m.recommendations
        f = data.fields
        h = data.test.holdout
        hu, hi_, hf = h[f.userid].values, h[f.itemid].values, h[f.feedback].values.astype(np.float64)
        hu = np.unique(hu, return_inverse=True)[1]
        n_items = data.get_test_shape()[1] if hasattr(data, 'get_test_shape') else recs.max() + 1
        p = cid + '/'
        out.update({p + 'recs': np.asarray(recs, dtype=np.int64), p + 'hu': hu.astype(np.int64), p + 'hi': hi_.astype(np.int64),
                    p + 'hf': hf, p + 'n_items': np.int64(n_items), p + 'holdout_size': np.int64(data.holdout_size)})
        for topk in T.METRIC_TOPKS:
            for sp in T.METRIC_SWITCH:
                want = dict((type(s).__name__, s) for s in quiet(ref_m.evaluate, 'all', topk=topk, switch_positive=sp))
                q = '%s%d_%s/' % (p, topk, sp)
                out[q + 'families'] = np.array(sorted(want))
                out[q + 'hits'] = hits_array(want['Hits'])
                out[q + 'coverage'] = np.float64(want['Experience'].coverage)
                for name, v in want['Ranking']._asdict().items():
                    if name in ('map', 'arhr', 'mrr'):
                        out[q + 'ranking_' + name] = np.float64(v)
                if 'hr' in want['Relevance']._asdict():
                    out[q + 'relevance_hr'] = np.float64(want['Relevance'].hr)
    for sp in (None, 3):
        recs, hu, hi_, hf, n_items, topk, per = T.zero_feedback_inputs()
        holdout = pd.DataFrame({'userid': hu, 'itemid': hi_, 'rating': hf})
        is_positive = None if sp is None else (hf >= sp)
        sd = rev.assemble_scoring_matrices(recs, holdout, 'userid', 'itemid', is_positive, feedback='rating')
        q = 'zero_%s/' % sp
        out[q + 'hits'] = hits_array(rev.get_hits(*sd, not_rated_penalty=1 if sp is None else 0))
        out[q + 'map'] = np.float64(rev.get_map_score(sd[1], sd[3], topk))
        out[q + 'arhr'] = np.float64(rev.get_arhr_score(sd[1]))
        out[q + 'hr'] = np.float64(rev.get_hr_score(sd[1]).hr)
        out[q + 'mrr'] = np.float64(rev.get_mrr_score(sd[1]))
    np.savez_compressed(os.path.join(HERE, 'dropin_metrics.npz'), **out)
    print('wrote tests/golden/dropin_metrics.npz (%d arrays)' % len(out))


if __name__ == '__main__':
    main()
