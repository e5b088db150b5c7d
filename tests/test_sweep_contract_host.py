"""The checker of the sweep's contract (sweep_contract_reference.py) on the CPU: lists made from the exact fp64 scores pass,
and each of five doctored lists fails under the name of the condition it breaks — a checker that accepted one of them would
let the device tests of test_gpu_sweep_instances.py pass on a sweep that is wrong in exactly that way."""
import numpy as np
import pytest

import rescore_settle_reference as R
import sweep_contract_reference as C

N_USERS, N_ITEMS, K, KC = 37, 333, 20, 16     # two groups (the last with 5 live users), 11 tiles (the last with 13 items)
EMPTY_USER, FEW_USER = 4, 33


def make_case():
    V = R.decaying_catalogue(5, N_ITEMS, K, cone=0.25)
    ip, ix, va = R.random_csr(np.random.RandomState(6), N_USERS, N_ITEMS, 5, 40, R.popularity(N_ITEMS))
    rows = [ix[ip[u]:ip[u + 1]] for u in range(N_USERS)]
    rows[EMPTY_USER] = rows[EMPTY_USER][:0]
    rows[FEW_USER] = np.sort(np.random.RandomState(7).choice(N_ITEMS, size=N_ITEMS - 5, replace=False)).astype(np.int32)
    ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ix = np.concatenate(rows).astype(np.int32)
    va = np.random.RandomState(8).randint(1, 6, size=len(ix)).astype(np.float32)
    return V, R.fold(ip, ix, va, V), ip, ix


@pytest.fixture(scope='module')
def setup():
    V, E, ip, ix = make_case()
    ref = C.SweepContract(V, E, (ip, ix))
    layouts = {'single': [C.all_tiles(N_ITEMS)], 'splits': [C.split_tiles(N_ITEMS, h, 3) for h in range(3)]}
    return ref, ip, ix, layouts


def test_exact_lists_pass(setup):
    ref, ip, ix, layouts = setup
    for name, tiles in layouts.items():
        cs, ci = ref.exact_lists(KC, tiles)
        assert cs.shape == (len(tiles), 64, KC)
        assert ref.check(KC, cs, ci, tiles) <= 2.0 ** -23 / ref.rel      # only the float32 rounding of the scores
    # the few-unseen user's list is short and complete, the empty row's list is full of zero scores
    cs, ci = ref.exact_lists(KC, layouts['single'])
    assert (ci[0, FEW_USER] >= 0).sum() == 5 and (cs[0, EMPTY_USER] == 0).all() and (ci[0, EMPTY_USER] >= 0).all()
    # without a filter the same users' lists hold seen items: they pass only against the unfiltered universe
    nof = ref.without_filter()
    cs, ci = nof.exact_lists(KC, layouts['single'])
    nof.check(KC, cs, ci, layouts['single'])
    with pytest.raises(C.ContractViolation) as e:
        ref.check(KC, cs, ci, layouts['single'])
    assert e.value.condition == 'C1'


def ordinary_user(ref, ip):
    """a user with plenty of unseen items whose KC-th and (KC+1)-th exact scores are far enough apart for doctoring 4"""
    for u in range(N_USERS):
        if u in (EMPTY_USER, FEW_USER):
            continue
        s = np.sort(np.where(ref.seen_mask[u], -np.inf, ref.exact[u]))[::-1]
        if s[KC - 1] - s[KC] > 4 * ref.bound_max[u] + abs(s[KC]) * 2.0 ** -14 and ip[u + 1] > ip[u]:
            return u
    raise AssertionError('no user with a clear gap at the list boundary')


@pytest.mark.parametrize('doctoring,condition', [('seen_item', 'C1'), ('duplicate', 'C1'), ('score_moved', 'C2'),
                                                 ('boundary_swapped', 'C3'), ('short_list', 'C3')])
def test_doctored_lists_fail_under_the_right_name(setup, doctoring, condition):
    ref, ip, ix, layouts = setup
    tiles = layouts['single']
    cs, ci = ref.exact_lists(KC, tiles)
    u = ordinary_user(ref, ip)
    if doctoring == 'seen_item':
        j = int(ix[ip[u]])
        ci[0, u, 3], cs[0, u, 3] = j, np.float32(ref.exact[u, j])
    elif doctoring == 'duplicate':
        ci[0, u, 5], cs[0, u, 5] = ci[0, u, 2], cs[0, u, 2]
    elif doctoring == 'score_moved':
        j = int(ci[0, u, 7])
        cs[0, u, 7] = np.float32(ref.exact[u, j] + 3 * ref.bound[u, j])
    elif doctoring == 'boundary_swapped':
        s = np.where(ref.seen_mask[u], -np.inf, ref.exact[u])
        s[ci[0, u]] = -np.inf
        j = int(np.argmax(s))                          # the best item the list leaves out takes the last slot
        ci[0, u, KC - 1], cs[0, u, KC - 1] = j, np.float32(ref.exact[u, j])
    elif doctoring == 'short_list':
        assert (~ref.seen_mask[u]).sum() >= KC
        ci[0, u, KC - 2:], cs[0, u, KC - 2:] = -1, -np.inf
    with pytest.raises(C.ContractViolation) as e:
        ref.check(KC, cs, ci, tiles)
    assert e.value.condition == condition, str(e.value)
    assert 'user %d' % u in str(e.value)
    # with the completeness condition switched off (raw lists of a two-phase sweep) C1 and C2 still hold
    if condition == 'C3':
        ref.check(KC, cs, ci, tiles, completeness=False)
    else:
        with pytest.raises(C.ContractViolation) as e:
            ref.check(KC, cs, ci, tiles, completeness=False)
        assert e.value.condition == condition


def test_split_lists_are_checked_against_their_own_tiles(setup):
    ref, ip, ix, layouts = setup
    tiles = layouts['splits']
    cs, ci = ref.exact_lists(KC, tiles)
    u = ordinary_user(ref, ip)
    cs[[0, 1], u], ci[[0, 1], u] = cs[[1, 0], u], ci[[1, 0], u]      # the lists of two splits exchanged
    with pytest.raises(C.ContractViolation) as e:
        ref.check(KC, cs, ci, tiles)
    assert e.value.condition == 'C1' and 'does not own' in str(e.value)


def test_merged_best_is_score_descending_item_ascending():
    ws = np.array([[[3.0, 1.0]], [[3.0, 2.0]], [[-np.inf, -np.inf]]], dtype=np.float32)
    wi = np.array([[[9, 4]], [[2, 7]], [[-1, -2]]], dtype=np.int32)
    s, i = C.merged_best(2, ws, wi, 1)
    assert i.tolist() == [[2, 9]] and s.tolist() == [[3.0, 3.0]]
    s, i = C.merged_best(8, ws, wi, 1)
    assert i.tolist() == [[2, 9, 7, 4, -1, -1, -1, -1]] and np.isneginf(s[0, 4:]).all()
