"""Generates tests/golden/lce_*.npz from the REFERENCE ITSELF: the unmodified `LCEModel` (hybrid/models.py:120-225) and
`LCEModelItemColdStart` (coldstart/models.py:122-146) of evfro/polara with their solver (lib/optimize.py:309-391), driven
on seeded data of the size of make_golden_coldstart.py through `RecommenderData` / `ItemColdStartData`.

The item column is called `item`: the reference's LCE(cs) reads `factors['item_features']` while its LCE writes
`factors[f'{itemid}_features']`, so the unmodified reference only runs under that name.

Stand-ins (test-only): numba, scikit-sparse and an empty `lightfm`, as in make_golden_coldstart.py.  The reference's solver
keeps its objective history to itself; it is recorded here by wrapping `polara.lib.optimize.trace` and `numpy.trace` for
the duration of a build and putting the recorded terms together with the reference's own expression (optimize.py:374-379),
and checked against the values the solver prints from its second pass on.

Stored: the inputs as the hot path sees them (training triplets, the one-hot matrices of the training and the cold items as
triplets, the reference's kNN graph as triplets, the holdout), the initial factors (the seeded draw of optimize.py:323-326),
W, Hu, Hs, the objective history, the dense scores of a few rows, the lists and the reference's evaluate() numbers.

Asserted for every fixture, so that equality is a fair demand (seeds are tried until the reference alone meets them): the
smallest gap between consecutive scores among each row's top-(k+1), relative to the row's largest score, is >= 1e-6; at
every pass the objective delta and `tolerance` differ by a factor >= 1.01; cond(Hs Hs^T) <= 1e6.

usage:  python tests/golden/make_golden_lce.py
"""
import contextlib
import io
import os
import re
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

from polara.recommender.data import RecommenderData
from polara.recommender.coldstart.data import ItemColdStartData
from polara.recommender.coldstart.models import LCEModelItemColdStart
from polara.recommender.hybrid.models import LCEModel
from polara.lib import optimize
from polara.lib.similarity import stack_features

TOPK, SCORE_ROWS = 10, 6
N_USERS, N_ITEMS, N_LABELS = 300, 150, 40


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def ratings(seed):
    rng = np.random.RandomState(seed)
    rows = [(u, int(it), float(rng.randint(1, 6))) for u in range(N_USERS)
            for it in rng.choice(N_ITEMS, rng.randint(6, 30), replace=False)]
    return pd.DataFrame(rows, columns=['userid', 'item', 'rating'])


def features(seed):
    rng = np.random.RandomState(seed)
    rows = [sorted(int(x) for x in rng.choice(N_LABELS, rng.randint(1, 6), replace=False)) for _ in range(N_ITEMS)]
    return pd.DataFrame({'genres': rows}, index=pd.Index(np.arange(N_ITEMS), name='item'))


def make_data(df, feat, cold_start, seed, test_sample=None):
    if cold_start:
        data = ItemColdStartData(df, 'userid', 'item', 'rating', seed=seed, item_features=feat)
    else:
        data = RecommenderData(df, 'userid', 'item', 'rating', seed=seed)
        data.warm_start = False
        data.holdout_size = 3
    data.verbose = False
    if test_sample is not None:
        data.test_sample = test_sample
    quiet(data.prepare)
    if cold_start:
        # keys of the holdout = row numbers of the lists (see make_golden_coldstart.py)
        new = data.index.itemid.cold_start.new.values
        if not np.array_equal(new, np.arange(len(new))):
            pos = pd.Series(np.arange(len(new)), index=new)
            hold = data.test.holdout
            hold['item_cold'] = hold['item_cold'].map(pos).values
    return data


class Recorder:
    """the arguments-free record of one build of the reference: every value its `trace` helper and `np.trace` return, the
    graph it built, and what it printed"""

    def __enter__(self):
        self.values, self.graphs = [], []
        self._trace, self._nptrace, self._graph = optimize.trace, np.trace, LCEModel.build_item_graph
        rec = self

        def trace(A, B):
            v = rec._trace(A, B)
            rec.values.append(float(v))
            return v

        def nptrace(*a, **kw):
            v = rec._nptrace(*a, **kw)
            rec.values.append(float(v))
            return v

        def graph(model, item_features, n_neighbors):
            A = rec._graph(model, item_features, n_neighbors)
            rec.graphs.append(A.copy())
            return A
        optimize.trace, np.trace, LCEModel.build_item_graph = trace, nptrace, graph
        self.out = io.StringIO()
        self._redirect = contextlib.redirect_stdout(self.out)
        self._redirect.__enter__()
        return self

    def __exit__(self, *exc):
        self._redirect.__exit__(*exc)
        optimize.trace, np.trace, LCEModel.build_item_graph = self._trace, self._nptrace, self._graph
        return False

    def history(self, alpha, beta, lamb):
        """optimize.py:374-379 on the recorded terms: two constants, then nine values per pass in the order of the calls"""
        v = self.values
        trXs, trXu, per = v[0], v[1], v[2:]
        assert len(per) % 9 == 0
        gamma = 1. - alpha
        hist = []
        for p in range(len(per) // 9):
            hs_x, hs_w, hu_x, hu_w, w_dw, w_aw, tr_w, hs_hs, hu_hu = per[9 * p:9 * p + 9]
            tr1 = alpha * (trXs - 2. * hs_x + hs_w)
            tr2 = gamma * (trXu - 2. * hu_x + hu_w)
            tr3 = beta * (w_dw - w_aw)
            tr4 = lamb * (tr_w + hs_hs + hu_hu)
            hist.append(tr1 + tr2 + tr3 + tr4)
        printed = [float(x) for x in re.findall(r'Objective:\s+(\S+)\s+Delta', self.out.getvalue())]
        assert printed == hist[1:], 'the recorded objective is not the one the reference printed'
        return np.array(hist)


def check_gaps(scores, topk, name):
    top = -np.sort(-scores, axis=1)[:, :topk + 1]
    scale = np.abs(scores).max(axis=1)
    ok = scale > 0
    gap = ((top[ok, :-1] - top[ok, 1:]).min(axis=1) / scale[ok]).min()
    assert gap >= 1e-6, '%s: relative score gap %.2e' % (name, gap)
    return gap


def eval_numbers(model):
    out = {}
    for s in quiet(model.evaluate, 'all'):
        for f, v in zip(s._fields, s):
            if v is not None:
                out['eval_%s_%s' % (type(s).__name__, f)] = np.float64(v)
    return out


def run(name, df, feat, cold_start, data_seed, seed, rank=10, tolerance=None, binary=True, test_sample=None, stop_window=None):
    data = make_data(df, feat, cold_start, data_seed, test_sample)
    model = (LCEModelItemColdStart if cold_start else LCEModel)(data, item_features=feat)
    model.verbose = False
    model.rank, model.topk, model.seed = rank, TOPK, seed
    model.binary_features = binary
    model.show_error = True                        # the solver prints its objective: checked against the record
    if tolerance is not None:
        model.tolerance = tolerance
    with Recorder() as rec:
        model.build()
    hist = rec.history(model.alpha, model.beta, model.regularization)
    deltas = np.abs(np.diff(hist))
    ratio = np.maximum(deltas / model.tolerance, model.tolerance / deltas)
    assert ratio.min() >= 1.01, '%s: an objective delta within a factor %.4f of the tolerance' % (name, ratio.min())
    if stop_window is not None:
        assert stop_window[0] <= len(hist) <= stop_window[1], '%s: stopped after %d passes' % (name, len(hist))
    userid, itemid = data.fields.userid, data.fields.itemid
    W, HuT, HsT = (np.asarray(model.factors[k], np.float64) for k in (itemid, userid, f'{itemid}_features'))
    cond = np.linalg.cond(HsT.T @ HsT)
    assert cond <= 1e6, '%s: cond(Hs Hs^T) = %.2e' % (name, cond)
    n, v1, v2 = W.shape[0], HsT.shape[0], HuT.shape[0]
    rs = np.random.RandomState(seed)
    W0, Hs0, Hu0 = rs.rand(n, rank), rs.rand(rank, v1), rs.rand(rank, v2)           # optimize.py:323-326
    A = rec.graphs[0].tocoo()
    if cold_start:
        cold_meta = model.item_features.reindex(data.index.itemid.cold_start.old.values, fill_value=[])
        scores = model.slice_recommendations(cold_meta, 0, cold_meta.shape[0])
        train_items = data.index.itemid.training.old.values
    else:
        test_data, test_shape, test_users = model._get_test_data()
        scores, _ = model.slice_recommendations(test_data, test_shape, 0, test_shape[0], test_users)
        seen = model.get_test_matrix(test_data, test_shape)[0].tocoo()
        scores = np.array(scores, np.float64)
        scores[seen.row, seen.col] = scores.min() - 1.       # the lists are over unseen items: so are the gaps
        train_items = data.index.itemid.old.values
    gap = check_gaps(np.asarray(scores, np.float64), TOPK, name)
    recs = np.asarray(model.get_recommendations(), np.int64)
    Ft, labels = stack_features(model.item_features.reindex(train_items, fill_value=[]), normalize=False)
    assert labels == model.item_features_labels
    Ft = Ft.tocoo()
    idx, val, shp = data.to_coo(tensor_mode=False)
    hold = data.test.holdout
    out = dict(model=np.str_(model.method), cold_start=np.bool_(cold_start), rank=np.int64(rank), topk=np.int64(TOPK),
               seed=np.int64(seed), alpha=np.float64(model.alpha), beta=np.float64(model.beta),
               regularization=np.float64(model.regularization), tolerance=np.float64(model.tolerance),
               max_iterations=np.int64(model.max_iterations), max_neighbours=np.int64(model.max_neighbours),
               binary_features=np.bool_(binary), W0=W0, Hs0=Hs0, Hu0=Hu0, W=W, Hu=HuT.T.copy(), Hs=HsT.T.copy(), objective=hist,
               scores=np.asarray(model.slice_recommendations(cold_meta, 0, SCORE_ROWS) if cold_start else
                                 model.slice_recommendations(test_data, test_shape, 0, SCORE_ROWS, test_users)[0], np.float64),
               recs=recs, min_rel_gap=np.float64(gap), cond_gram=np.float64(cond), min_delta_ratio=np.float64(ratio.min()),
               train_idx=idx.astype(np.int64), train_val=np.asarray(val, np.float64), train_shape=np.array(shp, np.int64),
               ft_row=Ft.row.astype(np.int32), ft_col=Ft.col.astype(np.int32), ft_shape=np.array(Ft.shape, np.int64),
               graph_row=A.row.astype(np.int32), graph_col=A.col.astype(np.int32), graph_val=A.data.astype(np.float64),
               graph_shape=np.array(A.shape, np.int64), hold_user=hold['userid'].values.astype(np.int64),
               hold_fdbk=hold['rating'].values.astype(np.float64))
    if cold_start:
        Fc = stack_features(cold_meta, labels=labels, normalize=False)[0].tocoo()
        out.update(fc_row=Fc.row.astype(np.int32), fc_col=Fc.col.astype(np.int32), fc_shape=np.array(Fc.shape, np.int64),
                   hold_cold=hold['item_cold'].values.astype(np.int64), n_cold=np.int64(Fc.shape[0]))
        if data.representative_users is not None:
            out['repr_users'] = data.representative_users.new.values.astype(np.int64)
    else:
        out.update(hold_item=hold['item'].values.astype(np.int64), test_users=np.asarray(test_users, np.int64))
    out.update(eval_numbers(model))
    return out


def early_tolerance(df, feat, data_seed, seed):
    """A tolerance the reference's own deltas put between two passes: the deltas first rise, then fall, so the tolerance is
    the geometric mean of the smallest delta so far and the first one that falls clearly below it — the pass it stops at."""
    data = make_data(df, feat, False, data_seed)
    model = LCEModel(data, item_features=feat)
    model.verbose, model.seed, model.show_error = False, seed, True
    with Recorder() as rec:
        model.build()
    deltas = np.abs(np.diff(rec.history(model.alpha, model.beta, model.regularization)))
    for j in range(1, len(deltas)):
        low = deltas[:j].min()
        if deltas[j] * 1.05 < low:
            return float(np.sqrt(deltas[j] * low))
    raise AssertionError('no pass whose delta falls below all earlier ones')


def make_all(s):
    df, feat = ratings(s), features(s + 1)
    data_seed, seed = 7, 100 + s
    out = [('lce_std', run('lce_std', df, feat, False, data_seed, seed, stop_window=(16, 16)))]
    tol = early_tolerance(df, feat, data_seed, seed)
    out.append(('lce_std_early', run('lce_std_early', df, feat, False, data_seed, seed, tolerance=tol, stop_window=(4, 10))))
    out.append(('lce_cs', run('lce_cs', df, feat, True, data_seed, seed)))
    out.append(('lce_cs_repr', run('lce_cs_repr', df, feat, True, data_seed, seed, test_sample=100)))
    out.append(('lce_std_distance', run('lce_std_distance', df, feat, False, data_seed, seed, binary=False)))
    out.append(('lce_cs_rank7', run('lce_cs_rank7', df, feat, True, data_seed, seed, rank=7)))
    return out


def main():
    for s in range(31, 80):
        try:
            made = make_all(s)
        except AssertionError as exc:
            print('seed %d rejected: %s' % (s, exc))
            continue
        for name, out in made:
            out['ratings_seed'] = np.int64(s)
            path = os.path.join(HERE, name + '.npz')
            np.savez_compressed(path, **out)
            print('%-18s %-8s passes %2d, gap %.1e, cond %.1f, delta ratio %.2f, %d bytes' % (
                name, out['model'], len(out['objective']), float(out['min_rel_gap']), float(out['cond_gram']),
                float(out['min_delta_ratio']), os.path.getsize(path)))
        return
    raise SystemExit('no seed met the conditions')


if __name__ == '__main__':
    main()
