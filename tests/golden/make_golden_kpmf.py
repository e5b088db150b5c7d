"""Generates tests/golden/kpmf_*.npz from the REFERENCE ITSELF: the unmodified `KernelizedPMF` (recommender/hybrid/models.py:
47-117) of evfro/polara with its optimizer (lib/optimize.py: kernelized_pmf_sgd -> mf_sgd_boilerplate -> generalized_sgd_sweep
with sparse_kernel_update), driven on the seeded ratings of make_golden_lce.py (300 users x 150 items, about 5 000 ratings)
through `SimilarityDataModel`, with the item cosine similarity of make_golden_hybrid.item_similarity and a seeded random
symmetric user relation, under the stand-ins of those generators (numba's decorators are no-ops).

`model.optimizer` is wrapped to record the interactions and the kernel matrices the model hands over.  For the blocked fixture
(kpmf_aligned_b4) the relations are masked to pairs of the same part of the B = 4 schedule — asserted on the RECORDED kernels —
and the wrapper permutes the interactions with `polara_amd.pmf.block_schedule` before it calls the unmodified optimizer: with
no kernel edge across parts a blocked epoch is the reference's own sweep on that permuted list, the one case where the
reference itself is the oracle for B > 1.

As in make_golden_pmf.py: model seeds are tried until the reference alone meets the conditions (relative score gaps >= 1e-6
among each row's top-(k+1) unseen items; `refined` and `tolerance` apart by a factor >= 1.01 at every epoch).  Then, NOT part
of the search (a miss stops the generator): the NumPy restatement of the device's arithmetic (tests/kpmf_reference.py) is
within 1e-12 x max|factor| of the reference in P, Q and the RMSE history.  The restatement differs from the reference in
rounding alone: the tree of `pm @ qn`, the canonical (sorted, duplicates summed) kernel rows, and the diagonal term added last.
That distance is stored as `restatement_gap`; the tests compare with the reference at 4 x restatement_gap.  The adaptive
fixtures run three epochs for the reason given in make_golden_pmf.py.

Also measured and printed (the general fixtures): the mean kernel degrees, the share of kernel edges that cross parts at B = 4,
and how far snapshot-only neighbour reads move P and Q after two epochs at B = 4.

usage:  python tests/golden/make_golden_kpmf.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from make_golden_lce import N_ITEMS, N_USERS, SCORE_ROWS, TOPK, check_gaps, eval_numbers, quiet, ratings   # the stand-ins, the reference
from make_golden_hybrid import item_similarity
from make_golden_pmf import ADAPTIVE_EPOCHS, Rejected

import numpy as np
import scipy.sparse as sps

from polara.lib import optimize
from polara.recommender.hybrid.data import SimilarityDataModel
from polara.recommender.hybrid.models import KernelizedPMF

import kpmf_reference as restated
from polara_amd.pmf import _parts, block_schedule


def user_relations(seed):
    """a seeded symmetric relation of the users: about 12 neighbours each, weights in (0, 1)"""
    rng = np.random.RandomState(seed)
    upper = sps.triu(sps.random(N_USERS, N_USERS, density=0.04, random_state=rng, format='csr'), k=1)
    return (upper + upper.T).tocsr()


def make_data(df, rel_users, rel_items, seed):
    data = SimilarityDataModel(df, 'userid', 'item', 'rating', seed=seed,
                               relations_matrices={'userid': rel_users, 'item': rel_items},
                               relations_indices={'userid': None if rel_users is None else np.arange(N_USERS),
                                                  'item': None if rel_items is None else np.arange(N_ITEMS)})
    data.warm_start = False
    data.holdout_size = 3
    data.verbose = False
    quiet(data.prepare)
    return data


def same_part_mask(data, blocks):
    """for both entities: [n x n] booleans in the ORIGINAL ids, True where the two lie in the same part of the schedule"""
    idx = data.training[[data.fields.userid, data.fields.itemid]].values
    out = []
    for entity, col, n in ((data.fields.userid, 0, N_USERS), (data.fields.itemid, 1, N_ITEMS)):
        part = _parts(np.bincount(idx[:, col], minlength=n), blocks, len(idx))
        index = data.get_entity_index(entity)
        part_of_old = np.empty(n, dtype=np.int64)
        part_of_old[index['old'].values] = part[index['new'].values]
        out.append(part_of_old[:, None] == part_of_old[None, :])
    return out


def crossing_share(K, part):
    K = K.tocoo()
    off = K.row != K.col
    return float((part[K.row[off]] != part[K.col[off]]).mean()) if off.any() else 0.


def run(name, df, rel_users, rel_items, data_seed, seed, blocks=1, rank=10, learn_rate=None, adjust=None, num_epochs=None,
        aligned=False):
    data = make_data(df, rel_users, rel_items, data_seed)
    if aligned:
        mu, mi = same_part_mask(data, blocks)
        data = make_data(df, rel_users.multiply(mu).tocsr(), rel_items.multiply(mi).tocsr(), data_seed)
    model = KernelizedPMF(data, seed=seed)
    model.verbose = False
    model.rank, model.topk = rank, TOPK
    if learn_rate is not None:
        model.learn_rate = learn_rate
    if num_epochs is not None:
        model.num_epochs = num_epochs
    rec = {}
    inner = model.optimizer
    assert inner is optimize.kernelized_pmf_sgd

    def optimizer(interactions, shape, nonzero_count, rank_, lrate, sigma, epochs, tol, kernel_matrices, **kwargs):
        u, i, v = (np.array(x) for x in interactions)
        key = u.astype(np.int64) * shape[1] + i
        assert (np.diff(key) > 0).all(), '%s: the interactions are not in row-major order' % name
        assert (v != 0).all()
        assert np.array_equal(nonzero_count[0], np.bincount(u, minlength=shape[0]))
        assert np.array_equal(nonzero_count[1], np.bincount(i, minlength=shape[1]))
        assert kwargs['kernel_update'] is None and kwargs['sparse_kernel_format'] is True
        perm, block_ptr = block_schedule(u, i, shape[0], shape[1], blocks)
        if blocks == 1:
            assert np.array_equal(perm, np.arange(len(u)))
        rec.update(u=u, i=i, v=v, shape=shape, perm=perm, block_ptr=block_ptr, kernels=tuple(K.copy() for K in kernel_matrices))
        return inner((u[perm], i[perm], v[perm]), shape, nonzero_count, rank_, lrate, sigma, epochs, tol, kernel_matrices, **kwargs)
    model.optimizer = optimizer
    quiet(model.build, **({'adjust_gradient': getattr(optimize, adjust)} if adjust else {}))
    n_users, n_items = (int(x) for x in rec['shape'])
    nnz = len(rec['v'])
    Ku, Ki = rec['kernels']
    upart = _parts(np.bincount(rec['u'], minlength=n_users), max(blocks, 4), nnz)
    ipart = _parts(np.bincount(rec['i'], minlength=n_items), max(blocks, 4), nnz)
    cross = (crossing_share(Ku, upart), crossing_share(Ki, ipart))
    if aligned:
        assert cross == (0., 0.), '%s: kernel edges cross the parts of the schedule' % name
        assert Ku.nnz > n_users and Ki.nnz > n_items, '%s: the masked kernels have no edges left' % name
    hist = np.array(model.rmse_history, np.float64)
    sse = hist ** 2 * nnz
    refined = np.abs(np.r_[np.finfo('f8').max, sse[:-1]] - sse) / np.r_[np.finfo('f8').max, sse[:-1]]
    ratio = np.maximum(refined / model.tolerance, model.tolerance / refined)
    if ratio.min() < 1.01:
        raise Rejected('%s: a refinement within a factor %.4f of the tolerance' % (name, ratio.min()))
    userid, itemid = data.fields.userid, data.fields.itemid
    P, Q = (np.asarray(model.factors[k], np.float64) for k in (userid, itemid))
    rs = np.random.RandomState(seed)
    P0 = rs.normal(scale=0.1, size=(n_users, rank))             # optimize.py:172-174
    Q0 = rs.normal(scale=0.1, size=(n_items, rank))
    test_data, test_shape, test_users = model._get_test_data()
    scores, _ = model.slice_recommendations(test_data, test_shape, 0, test_shape[0], test_users)
    seen = model.get_test_matrix(test_data, test_shape)[0].tocoo()
    masked = np.array(scores, np.float64)
    masked[seen.row, seen.col] = masked.min() - 1.              # the lists are over unseen items: so are the gaps
    try:
        score_gap = check_gaps(masked, TOPK, name)
    except AssertionError as exc:
        raise Rejected(str(exc))
    # the restatement of the device's arithmetic on the same schedule and the recorded kernels
    plan = restated.make_plan(rec['u'], rec['i'], rec['v'], n_users, n_items, blocks, Ku, Ki)
    assert np.array_equal(plan['perm'], rec['perm']) and np.array_equal(plan['block_ptr'], rec['block_ptr'])
    rP, rQ, rhist = restated.solve(plan, P0, Q0, model.learn_rate, model.sigma, model.num_epochs, model.tolerance, adjust)
    assert len(rhist) == len(hist), '%s: the restatement stops after %d epochs, the reference after %d' % (name, len(rhist), len(hist))
    gap = max(np.abs(rP - P).max(), np.abs(rQ - Q).max(), np.abs(rhist - hist).max())
    scale = max(np.abs(P).max(), np.abs(Q).max())
    assert gap <= 1e-12 * scale, '%s: the restatement is %.2e from the reference (factors up to %.2f)' % (name, gap, scale)
    if not aligned and blocks == 1 and rel_users is not None:
        plan4 = restated.make_plan(rec['u'], rec['i'], rec['v'], n_users, n_items, 4, Ku, Ki)
        lP, lQ, _ = restated.solve(plan4, P0, Q0, model.learn_rate, model.sigma, 2, 0., adjust)
        sP, sQ, _ = restated.solve(plan4, P0, Q0, model.learn_rate, model.sigma, 2, 0., adjust, live=False)
        print('  %s: kernel degrees %.1f / %.1f, edges across parts at B = 4: %.2f / %.2f, snapshot-only reads move P, Q by %.1e '
              'after two epochs at B = 4' % (name, Ku.nnz / n_users, Ki.nnz / n_items, cross[0], cross[1],
                                             max(np.abs(lP - sP).max(), np.abs(lQ - sQ).max())))
    recs = np.asarray(model.get_recommendations(), np.int64)
    hold = data.test.holdout
    lengths = np.diff(rec['block_ptr'])
    out = dict(model=np.str_(model.method), rank=np.int64(rank), topk=np.int64(TOPK), seed=np.int64(seed), blocks=np.int64(blocks),
               adjust=np.str_(adjust or 'none'), learn_rate=np.float64(model.learn_rate), sigma=np.float64(model.sigma),
               num_epochs=np.int64(model.num_epochs), tolerance=np.float64(model.tolerance), gamma=np.float64(model.gamma),
               factor_sigma_user=np.float64(model.factor_sigma[userid]), factor_sigma_item=np.float64(model.factor_sigma[itemid]),
               train_idx=np.stack([rec['u'], rec['i']], axis=1).astype(np.int64), train_val=rec['v'].astype(np.float64),
               train_shape=np.array(rec['shape'], np.int64), perm=rec['perm'], block_ptr=rec['block_ptr'],
               P0=P0, Q0=Q0, P=P, Q=Q, rmse_history=hist, scores=np.asarray(scores[:SCORE_ROWS], np.float64), recs=recs,
               min_rel_gap=np.float64(score_gap), min_refined_ratio=np.float64(ratio.min()), restatement_gap=np.float64(gap),
               empty_blocks=np.int64((lengths == 0).sum()), longest_block=np.int64(lengths.max()),
               cross_users=np.float64(cross[0]), cross_items=np.float64(cross[1]),
               hold_user=hold[userid].values.astype(np.int64), hold_item=hold[itemid].values.astype(np.int64),
               hold_fdbk=hold['rating'].values.astype(np.float64), test_users=np.asarray(test_users, np.int64))
    for key, K in (('ku', Ku), ('ki', Ki)):                     # the kernels entry by entry in the reference's storage order
        K = sps.csr_matrix(K)
        rows = np.repeat(np.arange(K.shape[0]), np.diff(K.indptr))
        out.update({key + '_row': rows.astype(np.int32), key + '_col': K.indices.astype(np.int32), key + '_val': K.data.astype(np.float64)})
    for key, entity in (('rel_u', userid), ('rel_i', itemid)):  # the relations in the model's own id order
        R = data.get_relations_matrix(entity)
        if R is not None:
            R = R.tocoo()
            out.update({key + '_row': R.row.astype(np.int32), key + '_col': R.col.astype(np.int32), key + '_val': R.data.astype(np.float64)})
    out.update(eval_numbers(model))
    return out


FIXTURES = [('kpmf_std', dict()), ('kpmf_items_only', dict(no_users=True)), ('kpmf_aligned_b4', dict(blocks=4, aligned=True)),
            ('kpmf_adagrad', dict(learn_rate=0.05, adjust='adagrad', num_epochs=ADAPTIVE_EPOCHS)),
            ('kpmf_rmsprop', dict(learn_rate=0.05, adjust='rmsprop', num_epochs=ADAPTIVE_EPOCHS))]


def main(only=None):
    s, data_seed = 31, 7
    df = ratings(s)
    rel_users, rel_items = user_relations(s + 1), item_similarity(N_ITEMS, 40, s + 2, 'cosine')
    for name, kw in FIXTURES:
        if only and name not in only:
            continue
        kw = dict(kw)
        ru = None if kw.pop('no_users', False) else rel_users
        for seed in range(100 + s, 160 + s):
            try:
                out = run(name, df, ru, rel_items, data_seed, seed, **kw)
                break
            except Rejected as exc:
                print('model seed %d rejected: %s' % (seed, exc))
        else:
            raise SystemExit('%s: no model seed met the conditions' % name)
        out['ratings_seed'] = np.int64(s)
        path = os.path.join(HERE, name + '.npz')
        np.savez_compressed(path, **out)
        print('%-16s seed %d B %d %-8s epochs %2d, score gap %.1e, refined ratio %.2f, restatement gap %.1e (factors up to %.2f), '
              '%d bytes' % (name, int(out['seed']), int(out['blocks']), str(out['adjust']), len(out['rmse_history']),
                            float(out['min_rel_gap']), float(out['min_refined_ratio']), float(out['restatement_gap']),
                            max(np.abs(out['P']).max(), np.abs(out['Q']).max()), os.path.getsize(path)))


if __name__ == '__main__':
    main(sys.argv[1:])
