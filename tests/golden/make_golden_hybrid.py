"""Generates tests/golden/hybrid_*.npz from the REFERENCE ITSELF: the unmodified `HybridSVD` / `ScaledHybridSVD` of
evfro/polara (hybrid/models.py:228-397) driven on seeded data through `SimilarityDataModel` (hybrid/data.py), with the
item similarity from the reference's own `polara.lib.similarity` of seeded binary item features.

scikit-sparse is not installed here: the test-only stand-in of tests/golden/_sksparse_shim provides `sksparse.cholmod`
(a dense NumPy factor under a seeded non-identity permutation).  Before anything is written, every fixture is made a
second time with the identity permutation and the two models are checked to agree (singular values, projectors up to
column signs, scores, lists): the invariance the device path relies on.

Stored: the inputs as the hot path sees them (training and test triplets, the relations matrix as triplets in the
model's item order), sigma, vl, vr, the dense scores of a few test users, the lists, and the lists after the
reference's rank truncation 10 -> 5 (`recs_rank5`).

usage:  python tests/golden/make_golden_hybrid.py
"""
import contextlib
import io
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, '_sksparse_shim'))
sys.path.insert(0, os.path.join(HERE, '_numba_shim'))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, ROOT)
warnings.filterwarnings('ignore')

import numpy as np
import pandas as pd
import scipy.sparse as sps

from sksparse import cholmod
from polara.recommender.hybrid.data import SimilarityDataModel
from polara.recommender.hybrid.models import HybridSVD, ScaledHybridSVD
from polara.lib.similarity import cosine_similarity, jaccard_similarity

RANK = 10
SCORE_USERS = 8


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def ratings(n_users, n_items, lo, hi, seed):
    rng = np.random.RandomState(seed)
    rows = []
    for u in range(n_users):
        for it in rng.choice(n_items, rng.randint(lo, hi), replace=False):
            rows.append((u, int(it), float(rng.randint(1, 6))))
    return pd.DataFrame(rows, columns=['userid', 'itemid', 'rating'])


def item_similarity(n_items, n_features, seed, kind):
    rng = np.random.RandomState(seed)
    F = sps.csr_matrix((rng.rand(n_items, n_features) < 0.08).astype(np.float64))
    F = F + sps.csr_matrix((np.ones(n_items), (np.arange(n_items), rng.randint(0, n_features, n_items))),
                           shape=F.shape)                      # no item without features
    F.data[:] = 1.0
    return (cosine_similarity if kind == 'cosine' else jaccard_similarity)(F.tocsr()).tocsr()


def run(df, S, model_cls, weight, warm_start, filter_seen, seed_perm, topk=10):
    cholmod.PERMUTATION_SEED = seed_perm
    n_items = S.shape[0]
    data = SimilarityDataModel(df, 'userid', 'itemid', 'rating', seed=0,
                               relations_matrices={'itemid': S, 'userid': None},
                               relations_indices={'itemid': np.arange(n_items), 'userid': None})
    data.verbose = False
    data.warm_start = warm_start
    data.holdout_size = 3
    quiet(data.prepare)
    model = model_cls(data)
    model.verbose = False
    model.rank = RANK
    model.topk = topk
    model.filter_seen = filter_seen
    model.features_weight = weight
    quiet(model.build)
    test_data, test_shape, _ = model._get_test_data()
    scores, _ = model.slice_recommendations(test_data, test_shape, 0, min(SCORE_USERS, test_shape[0]))
    recs = np.asarray(model.get_recommendations(), np.int64)
    vl, vr = model.get_item_projector()
    out = dict(model=np.str_(model.method), sigma=np.asarray(model.factors['singular_values'], np.float64),
               vl=np.asarray(vl, np.float64), vr=np.asarray(vr, np.float64), scores=np.asarray(scores, np.float64),
               recs=recs)
    model.rank = 5                                   # the reference's truncation (hybrid/models.py:327-336)
    out['recs_rank5'] = np.asarray(model.get_recommendations(), np.int64)
    out['builds_after_rank5'] = np.int64(len(model.training_time))
    rel = data.get_relations_matrix('itemid').tocoo()
    idx, val, shp = data.to_coo(tensor_mode=False)
    tu, ti, tf = test_data
    out.update(train_idx=idx.astype(np.int64), train_val=np.asarray(val, np.float64), train_shape=np.array(shp, np.int64),
               test_user=np.asarray(tu, np.int64), test_item=np.asarray(ti, np.int64), test_fdbk=np.asarray(tf, np.float64),
               test_shape=np.array(test_shape, np.int64), rel_row=rel.row.astype(np.int32), rel_col=rel.col.astype(np.int32),
               rel_val=rel.data.astype(np.float64), features_weight=np.float64(weight), topk=np.int64(topk),
               filter_seen=np.bool_(filter_seen), warm_start=np.bool_(warm_start), rank=np.int64(RANK))
    return out


def same_up_to_sign(a, b, tol):
    s = np.sign(np.sum(a * b, axis=0))
    return np.abs(a - b * s).max() <= tol * max(1.0, np.abs(a).max())


def check_invariance(a, b, name):
    assert np.allclose(a['sigma'], b['sigma'], rtol=1e-10, atol=0), name
    assert same_up_to_sign(a['vl'], b['vl'], 1e-9) and same_up_to_sign(a['vr'], b['vr'], 1e-9), name
    assert np.allclose(a['scores'], b['scores'], rtol=1e-9, atol=1e-10), name
    assert np.allclose(a['vr'] @ a['vl'].T, b['vr'] @ b['vl'].T, rtol=1e-9, atol=1e-12), name
    assert np.array_equal(a['recs'], b['recs']) and np.array_equal(a['recs_rank5'], b['recs_rank5']), name


def fixture(name, df, S, model_cls=HybridSVD, weight=0.5, warm_start=False, filter_seen=True, **extra):
    ident = run(df, S, model_cls, weight, warm_start, filter_seen, None)
    perm = run(df, S, model_cls, weight, warm_start, filter_seen, 12345)
    check_invariance(ident, perm, name)
    perm.update(extra)
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **perm)
    print('%-16s %s test %s, sigma[0] %.4f, %d bytes' % (name, perm['model'], tuple(perm['test_shape']), perm['sigma'][0],
                                                        os.path.getsize(path)))


def main():
    df = ratings(300, 120, 4, 20, seed=11)
    S = item_similarity(120, 40, seed=12, kind='cosine')
    fixture('hybrid_known', df, S)
    fixture('hybrid_nofilter', df, S, filter_seen=False)
    fixture('hybrid_warm', df, S, warm_start=True)
    fixture('hybrid_scaled', df, S, model_cls=ScaledHybridSVD)
    Sj = item_similarity(120, 40, seed=13, kind='jaccard')
    fixture('hybrid_weight_02', df, Sj, weight=0.2)
    fixture('hybrid_weight_09', df, Sj, weight=0.9)


if __name__ == '__main__':
    main()
