"""Contextual post-filtering without a GPU: the data class against the reference's mapped state (fixture made from the
reference itself, tests/golden/make_golden_contextual.py), the dense path and the model layer through the NumPy double, the
restatement of both orders, the refusals, the exports and the C prototype."""
import ctypes
import os
import re

import numpy as np
import pytest

import contextual_reference as cref
from conftest import ROOT, load_golden

import polara_amd
from polara_amd import _lib
from polara_amd.contextual import ItemPostFilteringMixin, check_context_lists
from polara_amd.data import ItemPostFilteringArrayData
from polara_amd.models import CoffeeModel, CooccurrenceModel, PopularityModel, SVDModel


class ContextualSVD(ItemPostFilteringMixin, SVDModel):
    pass


def fixture_data(g, **kw):
    shp = tuple(int(x) for x in g['train_shape'])
    contexts = [str(c) for c in g['contexts']]
    return ItemPostFilteringArrayData(
        (g['train_idx'][:, 0], g['train_idx'][:, 1], g['train_val']), n_users=shp[0], n_items=shp[1],
        holdout=(g['holdout_user'], g['holdout_item'], g['holdout_fdbk']), warm_start=False,
        item_context_mapping={c: (g['map_%s_item' % c], g['map_%s_value' % c]) for c in contexts},
        holdout_context={c: g['holdout_%s' % c] for c in contexts}, **kw)


@pytest.fixture(scope='module')
def g():
    return load_golden('contextual_small')


@pytest.fixture(scope='module')
def model(g):
    m = ContextualSVD(fixture_data(g), ops=cref.ContextNumpyOps())
    m.verbose = False
    m.rank, m.topk = int(g['rank']), int(g['topk'])
    m.build()
    return m


# ---- data class ---------------------------------------------------------------------------------------------------
def test_data_class_matches_the_reference_context_data(g):
    d = fixture_data(g)
    assert d.contexts == tuple(str(c) for c in g['contexts'])
    order = np.argsort(g['holdout_user'], kind='stable')
    for c in d.contexts:
        vals, ptr, items = d.context_values(c)
        uv = d.user_context(c)
        assert uv.dtype == np.int32 and len(uv) == len(order)
        ref_vals, ref_ptr, ref_items = g['ctx_%s_values' % c], g['ctx_%s_ptr' % c], g['ctx_%s_items' % c]
        ref_list = {v: np.sort(ref_items[ref_ptr[k]:ref_ptr[k + 1]]) for k, v in enumerate(ref_vals.tolist())}
        # value lists: every value of ours is one of the reference's with the same items; the reference's further values are empty
        for k, v in enumerate(vals.tolist()):
            mine = items[ptr[k]:ptr[k + 1]]
            assert len(mine) and np.array_equal(mine, np.unique(mine))
            if v in ref_list:
                assert np.array_equal(mine, ref_list[v]), (c, v)
        assert all(len(l) == 0 for v, l in ref_list.items() if v not in vals.tolist())
        # per-user values: test user r (sorted holdout users) has the list the reference maps its value to
        assert np.array_equal(g['ctx_%s_users' % c][order], np.sort(g['holdout_user']))
        for r, v in enumerate(g['ctx_%s_user_values' % c][order].tolist()):
            mine = items[ptr[uv[r]]:ptr[uv[r] + 1]] if uv[r] >= 0 else np.zeros(0, np.int64)
            assert np.array_equal(mine, ref_list[v]), (c, r)
    assert (d.user_context('daypart') == -1).any()          # the fixture's value 3 has no items: the reindex fill of the reference


def small_data(**kw):
    train = (np.array([0, 0, 1, 1, 2, 2]), np.array([0, 1, 1, 2, 3, 4]), np.ones(6))
    args = dict(n_users=3, n_items=5, holdout=(np.array([2, 0, 1]), np.array([0, 2, 3]), np.ones(3)),
                item_context_mapping={'a': (np.array([4, 1, 1, 9, -1, 3, 1]), np.array(['x', 'x', 'x', 'x', 'y', 'y', 'y'])),
                                      'b': (np.array([2, 0]), np.array([5, 5]))},
                holdout_context={'a': np.array(['y', 'x', 'z']), 'b': np.array([7, 5, 5])})
    args.update(kw)
    return ItemPostFilteringArrayData(train, **args)


def test_data_class_edges():
    d = small_data()
    vals, ptr, items = d.context_values('a')
    # unknown items (9, -1) dropped, the repeated pair (1, x) counted once, lists sorted
    assert vals.tolist() == ['x', 'y'] and ptr.tolist() == [0, 2, 4] and items.tolist() == [1, 4, 1, 3]
    # the holdout rows came unsorted (users 2, 0, 1): values follow their rows; 'z' is not in the mapping
    assert d.user_context('a').tolist() == [0, -1, 1]
    assert d.user_context('b').tolist() == [0, 0, -1] and d.context_values('b')[2].tolist() == [0, 2]
    with pytest.raises(ValueError):      # two holdout rows of one user
        small_data(holdout=(np.array([0, 0, 1]), np.array([2, 3, 3]), np.ones(3)))
    with pytest.raises(ValueError):      # values not aligned with the holdout rows
        small_data(holdout_context={'a': np.array(['y', 'x']), 'b': np.array([7, 5, 5])})
    with pytest.raises(ValueError):
        small_data(holdout_context={'a': np.array(['y', 'x', 'z'])})


def test_set_test_data_remaps_and_a_change_event_clears():
    d = small_data()
    before = d.context_data
    seen = []

    class Sub:
        def cb(self):
            seen.append(1)
    s = Sub()
    d.subscribe(d.on_update_event, s.cb)
    d.set_test_data(holdout=(np.array([1, 2]), np.array([0, 0]), np.ones(2)), holdout_context={'a': np.array(['x', 'x']), 'b': np.array([5, 1])})
    assert seen == [1] and d.context_data is not before
    assert d.user_context('a').tolist() == [0, 0] and d.user_context('b').tolist() == [0, -1]
    with pytest.raises(ValueError):      # the former values do not fit the new holdout
        d.set_test_data(holdout=(np.array([0, 1, 2]), np.array([2, 0, 0]), np.ones(3)))
    d.set_test_data(holdout=(np.array([1, 2]), np.array([0, 0]), np.ones(2)), holdout_context={'a': np.array(['x', 'y']), 'b': np.array([5, 1])})
    d.set_training_data((np.array([0, 1, 2]), np.array([0, 1, 2]), np.ones(3)))
    assert d._context is None                                 # dropped by the change event ...
    assert d.user_context('a').tolist() == [0, 1]             # ... and rebuilt on access


# ---- dense path and model layer through the NumPy double ---------------------------------------------------------------
def test_fixture_preconditions(g):
    assert g['min_plain_score'] > -1 and g['min_gap'] > 1e-9 and (g['scores'] != g['plain_scores']).any()
    assert (g['recs'] != g['plain_recs']).any(1).all()


def test_dense_path_reproduces_the_reference_block_and_lists(g, model):
    assert np.allclose(model.factors['singular_values'], g['singular_values'], rtol=1e-9)
    test_data, shape, test_users = model._get_test_data()
    assert tuple(shape) == tuple(g['test_shape']) and np.array_equal(test_users, g['test_users'])
    # the same known interactions as the reference's test users had (the order inside a user's row is free)
    assert np.array_equal(test_data[0], g['test_user']) and np.array_equal(test_data[2], g['test_fdbk'])
    assert np.array_equal(np.sort(test_data[0] * shape[1] + test_data[1]), np.sort(g['test_user'] * shape[1] + g['test_item']))
    scores, slice_data = model.slice_recommendations(test_data, shape, 0, shape[0], test_users)
    err = np.abs(scores - g['scores']).max() / np.abs(g['scores']).max()
    print('up-voted block: relative error %.3g' % err)
    assert err <= 1e-12
    model.downvote_seen_items(scores, slice_data)
    assert np.array_equal(model.get_topk_elements(scores), g['recs'])
    # a slice in the middle: M is the maximum of THAT block (the reference's chunk semantics)
    part, _ = model.slice_recommendations(test_data, shape, 5, 9)
    want = SVDModel.slice_recommendations(model, test_data, shape, 5, 9)[0]
    model.upvote_relevant_items(want, test_users[5:9])
    assert np.array_equal(part, want) and (part != SVDModel.slice_recommendations(model, test_data, shape, 5, 9)[0]).any()
    # the single-user convenience sees what a Polara user sees
    row, _ = model._user_scores(int(test_users[3]))
    assert row.shape == (1, shape[1]) and np.array_equal(model.get_topk_elements(row)[0], g['recs'][3])


def test_fused_path_through_the_double_equals_the_reference_lists(g, model):
    model.collect_recommend_stats = True
    recs = model.get_recommendations()
    assert np.array_equal(recs, g['recs'])
    cls = model.recommend_stats['context_class']
    assert cls.shape == recs.shape and cls.dtype == np.int32 and set(np.unique(cls)) <= {0, 1, 2, 3} and (cls > 0).any()
    assert (np.diff(cls, axis=1) <= 0).all()                 # classes never increase along a list
    model.collect_recommend_stats = False
    images = model._context_dev[1]
    assert np.array_equal(model.get_recommendations(), g['recs']) and model._context_dev[1] is images      # cached
    plain = SVDModel(model.data, ops=cref.ContextNumpyOps())
    plain.verbose = False
    plain.rank, plain.topk = model.rank, model.topk
    plain.build()
    assert np.array_equal(plain.get_recommendations(), g['plain_recs'])      # the plain model is untouched by the hook


# ---- restatement -------------------------------------------------------------------------------------------------
def test_literal_order_is_the_class_order_where_scores_exceed_minus_one():
    V, E, sp, si, ctx = cref.construction()
    scores = E @ V.T
    seen = cref.seen_mask(sp, si, *scores.shape)
    assert scores.min() > -1
    assert cref.min_gap(scores, seen, 10) > 1e-6       # the precondition, from the reference scores alone
    one = cref.literal_lists(scores, ctx, seen, 10)
    assert np.array_equal(cref.literal_lists(scores, ctx, seen, 10, chunk=64), one)
    ids, cls = cref.class_order_lists(scores, ctx, seen, 10)
    assert np.array_equal(ids, one)
    assert set(np.unique(cls)) == {0, 1, 2, 3}
    # and the tier-on-base form of the kernel's contract gives the same lists
    merged, mcls = cref.merge_reference(V, E, sp, si, ctx, cref.plain_lists(scores, seen, 10), scores=scores)
    assert np.array_equal(merged, ids) and np.array_equal(mcls, cls)
    merged, _ = cref.merge_reference(V, E, None, None, ctx, cref.plain_lists(scores, np.zeros_like(seen), 10), scores=scores)
    assert np.array_equal(merged, cref.class_order_lists(scores, ctx, np.zeros_like(seen), 10)[0])


def test_below_minus_one_the_literal_arithmetic_is_another_order():
    V, E, sp, si, ctx = cref.construction(gaussian=True)
    scores = E @ V.T
    seen = cref.seen_mask(sp, si, *scores.shape)
    assert scores.min() < -1
    ids, _ = cref.class_order_lists(scores, ctx, seen, 10)
    assert not np.array_equal(cref.literal_lists(scores, ctx, seen, 10), ids)


def test_list_checks_of_the_host_layer():
    ok = (np.array([0, -1, 1]), np.array([0, 2, 3]), np.array([1, 4, 0]))
    uv, ptr, items, longest = check_context_lists(*ok, 3, 5)
    assert uv.dtype == np.int32 and ptr.dtype == np.int64 and items.dtype == np.int32 and longest == 2
    empty = check_context_lists(np.array([-1]), np.array([0]), np.zeros(0), 1, 5)
    assert empty[2].tolist() == [0] and empty[3] == 0         # no entries: still an array with an address
    for bad in ((np.array([0, 2, 1]), ok[1], ok[2]),             # a value that does not exist
                (ok[0], np.array([0, 2, 4]), ok[2]),             # pointer past the entries
                (ok[0], ok[1], np.array([1, 5, 0])),             # item out of range
                (ok[0], ok[1], np.array([4, 1, 0])),             # descending inside a value
                (ok[0], ok[1], np.array([1, 1, 0]))):            # a duplicate
        with pytest.raises(ValueError):
            check_context_lists(*bad, 3, 5)
    with pytest.raises(ValueError):
        check_context_lists(*ok, 4, 5)


# ---- refusals, exports, ABI ----------------------------------------------------------------------------------------------
def test_refusals():
    d = small_data()
    for base in (CooccurrenceModel, PopularityModel, CoffeeModel):
        cls = type('Ctx' + base.__name__, (ItemPostFilteringMixin, base), {})
        with pytest.raises(NotImplementedError, match='contextual post-filtering'):
            cls(d, ops=cref.ContextNumpyOps())

    class TwoRanks:
        world, rank = 2, 0
    with pytest.raises(NotImplementedError, match='single-process'):
        ContextualSVD(d, ops=cref.ContextNumpyOps(), comm=TwoRanks())
    from polara_amd.data import ArrayData
    with pytest.raises(TypeError, match='ItemPostFilteringArrayData'):
        ContextualSVD(ArrayData((np.array([0, 1]), np.array([0, 1]), np.ones(2)), holdout=(np.array([0, 1]), np.array([1, 0]), np.ones(2))),
                      ops=cref.ContextNumpyOps())


def test_exports():
    assert polara_amd.ItemPostFilteringMixin is ItemPostFilteringMixin
    assert polara_amd.ItemPostFilteringArrayData is ItemPostFilteringArrayData
    assert {'ItemPostFilteringMixin', 'ItemPostFilteringArrayData'} <= set(polara_amd.__all__)
    assert 'ItemPostFiltering' in polara_amd.__doc__


def test_prototype_limits_and_argument_checks():
    header = open(os.path.join(ROOT, 'include', 'polara_hip.h')).read()
    for name in ('pk_context_merge_f64', 'pk_context_window', 'pk_context_max'):
        assert name in _lib.PROTOTYPES and re.search(r'\b%s\(' % name, header)
    import test_abi
    test_abi.test_python_prototypes_cover_the_header()
    lib = _lib.load()
    assert lib.pk_context_window() == 4096 and lib.pk_context_max() == 4
    three = (ctypes.c_void_p * 1)(8)
    one = ctypes.c_void_p(8)          # never dereferenced: every call below is refused before a launch

    def call(n_ctx=1, K=4, topk=10, V=one, base=one, out=ctypes.c_void_p(16), max_list=5):
        return lib.pk_context_merge_f64(None, 4, 50, K, V, K, one, K, None, None, n_ctx, three, three, three, max_list, base, topk, out,
                                        None, None)
    assert call(n_ctx=0) != 0 and call(n_ctx=5) != 0
    assert call(topk=0) != 0 and call(topk=1025) != 0
    assert call(K=0) != 0 and call(K=1025) != 0
    assert call(V=None) != 0 and call(base=None) != 0 and call(out=None) != 0
    assert call(out=one) != 0                                  # in place
    assert call(max_list=51) != 0
    assert b'pk_context_merge_f64' in lib.pk_last_error()
