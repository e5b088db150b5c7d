"""Generates tests/golden/contextual_small.npz from the REFERENCE ITSELF: the unmodified `ItemPostFilteringData` and
`ItemPostFilteringMixin` of evfro/polara (recommender/contextual/) over `SVDModel`, driven on small seeded implicit data with
two contexts; the inputs the hot path sees are stored next to the reference's mapped context data, its up-voted score block,
its lists and the lists of the plain model.

Runs only in the build container (imports the reference from /root/reference through the test-only numba shim, like
make_golden.py).  The script asserts what the tests rely on: the (single) chunk has up-voted entries, every plain score is
> -1 (where the reference's arithmetic is the class order), and no two neighbouring up-voted scores within ranks 1..11 of a
user are closer than 1e-9.

usage:  python tests/golden/make_golden_contextual.py
"""
import contextlib
import io
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, '_numba_shim'))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, ROOT)
warnings.filterwarnings('ignore')

import numpy as np
import pandas as pd

from polara.recommender.contextual.data import ItemPostFilteringData
from polara.recommender.contextual.models import ItemPostFilteringMixin
from polara.recommender.models import SVDModel

N_USERS, N_ITEMS, RANK, TOPK = 120, 60, 10, 10
GENRES = ['g%d' % g for g in range(6)]


class ContextualSVD(ItemPostFilteringMixin, SVDModel):
    pass


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def frames(seed):
    """Implicit interactions with a taste per user (three item clusters), a genre and a daypart on every row, and the two
    item-context mappings: genre (1-2 per item; the row carries one of its item's) and daypart (many to many, unrelated to
    the row's value; value 3 occurs on rows but has no items, and two pairs name items the data does not know)."""
    rng = np.random.RandomState(seed)
    item_genres = [sorted(rng.choice(len(GENRES), rng.randint(1, 3), replace=False)) for _ in range(N_ITEMS)]
    rows = []
    for u in range(N_USERS):
        taste = rng.randint(3)
        p = np.where(np.arange(N_ITEMS) % 3 == taste, 5.0, 1.0)
        items = rng.choice(N_ITEMS, rng.randint(8, 21), replace=False, p=p / p.sum())
        for it in items:
            rows.append((u, 100 + int(it), 1.0, GENRES[item_genres[it][rng.randint(len(item_genres[it]))]], int(rng.randint(4))))
    df = pd.DataFrame(rows, columns=['userid', 'itemid', 'rating', 'genre', 'daypart'])
    genre_map = pd.DataFrame([(100 + it, GENRES[g]) for it in range(N_ITEMS) for g in item_genres[it]], columns=['itemid', 'genre'])
    day_pairs = [(100 + it, d) for it in range(N_ITEMS) for d in range(3) if rng.rand() < 0.25]
    day_pairs += [(7000, 0), (7001, 2)]
    day_map = pd.DataFrame(day_pairs, columns=['itemid', 'daypart'])
    return df, {'genre': genre_map, 'daypart': day_map}


def hit_rate(recs, holdout_items):
    return float((recs == holdout_items[:, None]).any(1).mean())


def main(seed=3):
    df, mapping = frames(seed)
    data = ItemPostFilteringData(df, 'userid', 'itemid', 'rating', seed=0, item_context_mapping=mapping)
    data.verbose = False
    data.warm_start = False
    data.holdout_size = 1
    quiet(data.prepare)

    def build(cls):
        model = cls(data)
        model.verbose = False
        model.rank, model.topk = RANK, TOPK
        np.random.seed(0)
        quiet(model.build)
        return model

    plain, ctx = build(SVDModel), build(ContextualSVD)
    test_data, test_shape, test_users = ctx._get_test_data()
    n_test = int(test_shape[0])
    plain_scores, _ = plain.slice_recommendations(test_data, test_shape, 0, n_test, test_users)
    scores, slice_data = ctx.slice_recommendations(test_data, test_shape, 0, n_test, test_users)
    upvoted = scores != plain_scores
    recs, plain_recs = ctx.get_recommendations(), plain.get_recommendations()

    assert len(ctx._get_slices_idx(test_shape)) == 2, 'one chunk expected'
    assert upvoted.any(), 'the chunk has no up-voted entry'
    assert plain_scores.min() > -1, 'scores <= -1: the literal arithmetic is not the class order'
    down = scores.copy()
    ctx.downvote_seen_items(down, slice_data)
    head = -np.sort(-down, axis=1)[:, :TOPK + 1]
    gap = float((head[:, :-1] - head[:, 1:]).min())
    assert gap > 1e-9, 'neighbouring scores %g apart within ranks 1..%d' % (gap, TOPK + 1)

    hold = data.test.holdout
    item_new = data.index.itemid.set_index('old').new
    out = dict(rank=np.int64(RANK), topk=np.int64(TOPK), test_shape=np.array(test_shape, np.int64),
               test_users=np.asarray(test_users, np.int64), min_plain_score=np.float64(plain_scores.min()), min_gap=np.float64(gap),
               holdout_user=hold['userid'].values.astype(np.int64), holdout_item=hold['itemid'].values.astype(np.int64),
               holdout_fdbk=hold['rating'].values.astype(np.float64),
               scores=scores, plain_scores=plain_scores, recs=np.asarray(recs, np.int64), plain_recs=np.asarray(plain_recs, np.int64),
               singular_values=np.asarray(ctx.factors['singular_values'], np.float64),
               contexts=np.array(list(mapping), dtype=np.str_))
    idx, val, shp = data.to_coo(tensor_mode=False)
    out.update(train_idx=idx.astype(np.int64), train_val=np.asarray(val, np.float64), train_shape=np.array(shp, np.int64),
               test_user=np.asarray(test_data[0], np.int64), test_item=np.asarray(test_data[1], np.int64),
               test_fdbk=np.asarray(test_data[2], np.float64))
    for c, frame in mapping.items():
        # the mapping pairs in the data's item ids (-1: an item the data does not know)
        out['map_%s_item' % c] = frame['itemid'].map(item_new).fillna(-1).values.astype(np.int64)
        out['map_%s_value' % c] = frame[c].values
        out['holdout_%s' % c] = hold[c].values
        cd = data.context_data[c]
        user_data, item_data = cd['userid'], cd['itemid']
        out['ctx_%s_users' % c] = user_data.index.values.astype(np.int64)
        out['ctx_%s_user_values' % c] = user_data.values
        out['ctx_%s_values' % c] = item_data.index.values
        lists = [np.asarray(l, dtype=np.int64) for l in item_data.values]
        out['ctx_%s_ptr' % c] = np.r_[0, np.cumsum([len(l) for l in lists])].astype(np.int64)
        out['ctx_%s_items' % c] = np.concatenate(lists) if lists else np.zeros(0, np.int64)
    for k, v in out.items():
        v = np.asarray(v)
        out[k] = v.astype(np.str_) if v.dtype == object else v          # (pandas keeps strings as objects: no pickles in a fixture)
    path = os.path.join(HERE, 'contextual_small.npz')
    np.savez_compressed(path, **out)
    h = out['holdout_item'][np.argsort(out['holdout_user'], kind='stable')]
    print('contextual_small: test %s, %d up-voted entries, min plain score %.3g, min gap %.3g, HR@%d %.2f -> %.2f, '
          '%d/%d lists changed, %d bytes' % (tuple(test_shape), int(upvoted.sum()), plain_scores.min(), gap, TOPK,
                                             hit_rate(plain_recs, h), hit_rate(recs, h),
                                             int((recs != plain_recs).any(1).sum()), n_test, os.path.getsize(path)))


if __name__ == '__main__':
    main()
