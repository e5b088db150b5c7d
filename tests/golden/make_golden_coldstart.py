"""Generates tests/golden/coldstart_*.npz from the REFERENCE ITSELF: the unmodified item cold-start models of evfro/polara
(coldstart/models.py: PureSVD(cs), PureSVD(cs)-s, HybridSVD(cs), HybridSVD(cs)-s, MP(cs)) driven on seeded data through
`ItemColdStartData` / `ItemColdStartSimilarityData` (coldstart/data.py).

Stand-ins (test-only): numba, scikit-sparse (a dense NumPy factor under a seeded permutation) and an empty `lightfm`.
The hybrid fixtures are made twice — identity and seeded Cholesky permutation — and checked to agree (singular values, W up
to column signs, scores, lists) before anything is written.

Stored: the inputs as the hot path sees them (training triplets, the one-hot matrices of the training and the cold items
over the training labels as triplets, the relations of the training items as triplets, the holdout), sigma, U, V or vl / vr,
W, G, the dense scores of a few cold items, the lists, the lists after the reference's rank truncation 10 -> 5, and the
reference's evaluate() numbers.

Two conditions are asserted for every fixture, so that equality of lists is a fair demand: the smallest gap between
consecutive scores among each row's top-(k+1), relative to the row's largest score, is >= 1e-6, and cond(W^T W) <= 1e6.

usage:  python tests/golden/make_golden_coldstart.py
"""
import contextlib
import io
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for shim in ('_lightfm_shim', '_sksparse_shim', '_numba_shim'):
    sys.path.insert(0, os.path.join(HERE, shim))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, ROOT)
warnings.filterwarnings('ignore')

import numpy as np
import pandas as pd
import scipy.sparse as sps

from sksparse import cholmod
from polara.recommender.coldstart.data import ItemColdStartData, ItemColdStartSimilarityData
from polara.recommender.coldstart import models as cs
from polara.lib.similarity import stack_features, cosine_similarity

RANK, TOPK, SCORE_ITEMS = 10, 10, 6
N_USERS, N_ITEMS, N_LABELS = 300, 150, 40
ODD_UNKNOWN_ONLY, ODD_NO_LABELS, ODD_MIXED = 'only-unknown', 'none', 'mixed'


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def ratings(seed):
    rng = np.random.RandomState(seed)
    rows = [(u, int(it), float(rng.randint(1, 6))) for u in range(N_USERS)
            for it in rng.choice(N_ITEMS, rng.randint(6, 30), replace=False)]
    return pd.DataFrame(rows, columns=['userid', 'itemid', 'rating'])


def features(seed):
    rng = np.random.RandomState(seed)
    rows = [sorted(int(x) for x in rng.choice(N_LABELS, rng.randint(1, 6), replace=False)) for _ in range(N_ITEMS)]
    return pd.DataFrame({'genres': rows}, index=pd.Index(np.arange(N_ITEMS), name='itemid'))


def similarity(feat):
    F, _ = stack_features(feat, normalize=False)
    return cosine_similarity(F.tocsr().astype(np.float64)).tocsr()


def make_data(df, feat, hybrid, seed, test_sample=None):
    if hybrid:
        S = similarity(feat)
        data = ItemColdStartSimilarityData(df, 'userid', 'itemid', 'rating', seed=seed, item_features=feat,
                                           relations_matrices={'itemid': S, 'userid': None},
                                           relations_indices={'itemid': feat.index.values, 'userid': None})
    else:
        data = ItemColdStartData(df, 'userid', 'itemid', 'rating', seed=seed, item_features=feat)
    data.verbose = False
    if test_sample is not None:
        data.test_sample = test_sample
    quiet(data.prepare)
    # The validity filter of the data object drops cold items but leaves the numbers of the others as they were, so the
    # holdout's keys would no longer be row numbers of the lists (which follow the filtered cold-start index).  The keys
    # are renumbered here — the holdout frame of the reference's data object itself, before any model sees it — so that
    # the reference's evaluate() matches rows and keys.
    new = data.index.itemid.cold_start.new.values
    if not np.array_equal(new, np.arange(len(new))):
        pos = pd.Series(np.arange(len(new)), index=new)
        hold = data.test.holdout
        hold['itemid_cold'] = hold['itemid_cold'].map(pos).values
    return data


def eval_numbers(model):
    out = {}
    for s in quiet(model.evaluate, 'all'):
        for f, v in zip(s._fields, s):
            if v is not None:
                out['eval_%s_%s' % (type(s).__name__, f)] = np.float64(v)
    return out


def data_arrays(data, model):
    idx, val, shp = data.to_coo(tensor_mode=False)
    hold = data.test.holdout
    out = dict(train_idx=idx.astype(np.int64), train_val=np.asarray(val, np.float64), train_shape=np.array(shp, np.int64),
               hold_user=hold['userid'].values.astype(np.int64), hold_cold=hold['itemid_cold'].values.astype(np.int64),
               hold_fdbk=hold['rating'].values.astype(np.float64),
               n_cold=np.int64(data.index.itemid.cold_start.shape[0]),
               cold_old=data.index.itemid.cold_start.old.values.astype(np.int64))
    repr_users = data.representative_users
    if repr_users is not None:
        out['repr_users'] = repr_users.new.values.astype(np.int64)
    if getattr(model, 'item_features_labels', None) is not None:
        train = model.item_features.reindex(data.index.itemid.training.old.values, fill_value=[])
        Ft, labels = stack_features(train, stacked_index=False, normalize=False)
        assert labels == model.item_features_labels
        cold = model.item_features.reindex(data.index.itemid.cold_start.old.values, fill_value=[])
        Fc, _ = stack_features(cold, labels=labels, normalize=False)
        Ft, Fc = Ft.tocoo(), Fc.tocoo()
        out.update(ft_row=Ft.row.astype(np.int32), ft_col=Ft.col.astype(np.int32), ft_shape=np.array(Ft.shape, np.int64),
                   fc_row=Fc.row.astype(np.int32), fc_col=Fc.col.astype(np.int32), fc_shape=np.array(Fc.shape, np.int64))
    if hasattr(data, 'get_relations_matrix'):
        rel = data.get_relations_matrix('itemid').tocoo()
        out.update(rel_row=rel.row.astype(np.int32), rel_col=rel.col.astype(np.int32), rel_val=rel.data.astype(np.float64))
    return out


def check_gaps(scores, topk, name):
    """smallest gap between consecutive scores among each row's top-(k+1), relative to the row's largest score"""
    top = -np.sort(-scores, axis=1)[:, :topk + 1]
    scale = np.abs(scores).max(axis=1)
    ok = scale > 0
    gap = ((top[ok, :-1] - top[ok, 1:]).min(axis=1) / scale[ok]).min()
    assert gap >= 1e-6, '%s: relative score gap %.2e' % (name, gap)
    return gap


def run(model_cls, df, feat, data_seed, seed_perm=None, test_sample=None, name=''):
    cholmod.PERMUTATION_SEED = seed_perm
    hybrid = issubclass(model_cls, cs.HybridSVDItemColdStart)
    data = make_data(df, feat, hybrid, data_seed, test_sample)
    model = model_cls(data)
    model.verbose = False
    model.rank, model.topk = RANK, TOPK
    quiet(model.build)
    itemid, userid = data.fields.itemid, data.fields.userid
    cold_meta = model.item_features.reindex(data.index.itemid.cold_start.old.values, fill_value=[])
    n_cold = cold_meta.shape[0]
    all_scores = model.slice_recommendations(cold_meta, 0, n_cold)
    W, G = model.item_features_embeddings, model._item_features_transform_helper
    gap = check_gaps(all_scores, TOPK, name)
    cond = np.linalg.cond(W.T @ W)
    assert cond <= 1e6, '%s: cond(W^T W) = %.2e' % (name, cond)
    recs = np.asarray(model.get_recommendations(), np.int64)
    out = dict(model=np.str_(model.method), sigma=np.asarray(model.factors['singular_values'], np.float64),
               U=np.asarray(model.factors[userid], np.float64), W=np.asarray(W, np.float64), G=np.asarray(G, np.float64),
               scores=np.asarray(all_scores[:SCORE_ITEMS], np.float64), recs=recs, rank=np.int64(RANK), topk=np.int64(TOPK),
               min_rel_gap=np.float64(gap), cond_gram=np.float64(cond))
    if hybrid:
        vl, vr = model.get_item_projector()
        out.update(vl=np.asarray(vl, np.float64), vr=np.asarray(vr, np.float64), features_weight=np.float64(model.features_weight))
    else:
        out['V'] = np.asarray(model.factors[itemid], np.float64)
    out.update(eval_numbers(model))
    out.update(data_arrays(data, model))
    model.rank = 5
    check_gaps(model.slice_recommendations(cold_meta, 0, n_cold), TOPK, name + ' (rank 5)')
    out['recs_rank5'] = np.asarray(model.get_recommendations(), np.int64)
    out['G_rank5'] = np.asarray(model._item_features_transform_helper, np.float64)
    out['builds_after_rank5'] = np.int64(len(model.training_time))
    return out


def same_up_to_sign(a, b, tol):
    s = np.sign(np.sum(a * b, axis=0))
    return np.abs(a - b * s).max() <= tol * max(1.0, np.abs(a).max())


PENDING = []


def save(name, out):
    PENDING.append((name, out))


def write(name, out):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    print('%-26s %-16s cold %3d, gap %.1e, cond %.1f, %d bytes' % (name, out['model'], int(out['n_cold']),
          float(out.get('min_rel_gap', np.nan)), float(out.get('cond_gram', np.nan)), os.path.getsize(path)))


def hybrid_fixture(name, model_cls, df, feat, data_seed):
    ident = run(model_cls, df, feat, data_seed, None, name=name)
    perm = run(model_cls, df, feat, data_seed, 12345, name=name)
    assert np.allclose(ident['sigma'], perm['sigma'], rtol=1e-10, atol=0), name
    assert same_up_to_sign(ident['W'], perm['W'], 1e-9) and same_up_to_sign(ident['U'], perm['U'], 1e-9), name
    assert np.allclose(ident['scores'], perm['scores'], rtol=1e-9, atol=1e-12), name
    assert np.array_equal(ident['recs'], perm['recs']) and np.array_equal(ident['recs_rank5'], perm['recs_rank5']), name
    save(name, perm)


def odd_features(feat, df, data_seed):
    """three cold items changed: one keeps only a label no training item has, one loses all labels, one gets an unknown
    label next to its known ones.  The first two vanish from the reference's cold-start index."""
    probe = make_data(df, feat, False, data_seed)
    cold = probe.index.itemid.cold_start.old.values
    feat = feat.copy()
    a, b, c = (int(x) for x in cold[:3])
    feat.at[a, 'genres'] = [N_LABELS + 5]
    feat.at[b, 'genres'] = []
    feat.at[c, 'genres'] = list(feat.at[c, 'genres']) + [N_LABELS + 6]
    return feat, np.array([a, b, c], np.int64), len(cold)


def mp_fixture(name, df, feat, data_seed, test_sample):
    data = make_data(df, feat, False, data_seed, test_sample)
    model = cs.PopularityModelItemColdStart(data)
    model.verbose = False
    model.topk = TOPK
    quiet(model.build)
    recs = np.asarray(model.get_recommendations(), np.int64)
    activity = np.bincount(data.training['userid'].values, minlength=data.index.userid.training.shape[0])
    out = dict(model=np.str_(model.method), recs=recs, activity=activity.astype(np.int64), topk=np.int64(TOPK))
    out.update(eval_numbers(model))
    out.update(data_arrays(data, model))
    return out


def make_all(data_seed_ratings):
    df, feat = ratings(data_seed_ratings), features(data_seed_ratings + 1)
    seed = 7
    save('coldstart_svd', run(cs.SVDModelItemColdStart, df, feat, seed, name='coldstart_svd'))
    save('coldstart_svd_scaled', run(cs.ScaledSVDItemColdStart, df, feat, seed, name='coldstart_svd_scaled'))
    hybrid_fixture('coldstart_hybrid', cs.HybridSVDItemColdStart, df, feat, seed)
    hybrid_fixture('coldstart_hybrid_scaled', cs.ScaledHybridSVDItemColdStart, df, feat, seed)
    save('coldstart_repr', run(cs.SVDModelItemColdStart, df, feat, seed, test_sample=100, name='coldstart_repr'))
    odd, changed, n_before = odd_features(feat, df, seed)
    out = run(cs.SVDModelItemColdStart, df, odd, seed, name='coldstart_odd_features')
    assert int(out['n_cold']) == n_before - 2 and changed[2] in out['cold_old'] and changed[0] not in out['cold_old']
    # the inputs BEFORE the reference's validity filter: what ItemColdStartArrayData is given
    probe = make_data(df, feat, False, seed)
    hold = probe.test.holdout
    raw_feat = odd.reindex(probe.index.itemid.cold_start.old.values)
    labels_all = sorted({x for row in odd['genres'] for x in row})
    lab_id = {x: i for i, x in enumerate(labels_all)}
    tr = odd.reindex(probe.index.itemid.training.old.values)
    out.update(raw_hold_user=hold['userid'].values.astype(np.int64), raw_hold_cold=hold['itemid_cold'].values.astype(np.int64),
               raw_hold_fdbk=hold['rating'].values.astype(np.float64), raw_n_labels=np.int64(len(labels_all)),
               raw_cold_ptr=np.r_[0, np.cumsum([len(r) for r in raw_feat['genres']])].astype(np.int64),
               raw_cold_lab=np.array([lab_id[x] for r in raw_feat['genres'] for x in r], np.int64),
               raw_train_ptr=np.r_[0, np.cumsum([len(r) for r in tr['genres']])].astype(np.int64),
               raw_train_lab=np.array([lab_id[x] for r in tr['genres'] for x in r], np.int64),
               raw_cold_old=probe.index.itemid.cold_start.old.values.astype(np.int64), changed=changed)
    save('coldstart_odd_features', out)
    save('coldstart_mp', mp_fixture('coldstart_mp', df, feat, seed, None))
    save('coldstart_mp_repr', mp_fixture('coldstart_mp_repr', df, feat, seed, 100))


def main():
    # seeds are tried in order until every fixture meets the two conditions (no row of a fixture is excused as a tie)
    for s in range(31, 80):
        del PENDING[:]
        try:
            make_all(s)
        except AssertionError as exc:
            print('ratings seed %d rejected: %s' % (s, exc))
            continue
        for name, out in PENDING:
            out['ratings_seed'] = np.int64(s)
            write(name, out)
        return
    raise SystemExit('no seed met the conditions')


if __name__ == '__main__':
    main()
