"""Generates tests/golden/similarity_*.npz from the REFERENCE ITSELF: the unmodified `polara.lib.similarity` of evfro/polara
(`cosine_similarity`, `cosine_tfidf_similarity`, `jaccard_similarity`, `jaccard_similarity_weighted`) on seeded item features.

Runs only in the build container (imports the reference from /root/reference through the test-only numba stand-in, like
make_golden_sim.py).  Stored: the features as the CSR arrays they were generated with (stored order, explicit zeros kept),
the settings, and the reference's matrix made canonical (`tocsr()`, `sort_indices()`) with indptr, indices and data exact.

  similarity_wide_<kind>   2 597 items (one 2 048-column window, one 512-column wave quarter, 37), about 600 labels, 1-4 labels
                           per item; one item with 130 labels (three 64-entry chunks of a left row), one label carried by 300
                           items (a long row of F^T across both windows), five items without labels, two explicit zeros,
                           weights 2..5 on a fifth of the entries.  kinds: cosine, cosine-binary, tfidf-cosine, jaccard;
                           `fill0_*` / `fill1_*`: fill_diagonal False / True.  The Jaccard file holds `*_data` = the contract
                           (`_jaccard_similarity_inplace` on the fp64 count F01.astype(float64).dot(F01.T)) and
                           `*_data_as_run` (`jaccard_similarity` as the installed SciPy runs it: a boolean product, every
                           count 1); the two are asserted to differ.
  similarity_cross         70 further items against the 2 597: the block [2597:, :2597] of the reference's matrices over the
                           stacked features, per kind.
  similarity_wj            weighted Jaccard on 2 100 items (crosses a window; the interpreted reference loop takes a minute);
                           its last 60 items against the first 2 040 are the cross case of the tests.
  similarity_wj_nofill     the same with fill_diagonal=False (the explicit 0.0 the reference's setdiag leaves on the diagonal
                           of an item without labels is dropped: see without_stored_zeros).
  similarity_wj_small      150 items, both settings: what a host test can afford to restate.

Conditions asserted before anything is written: stored entries in both windows and on both sides of a 512-column quarter
boundary, bitwise symmetry of the symmetric matrices, finite values, the restatement of tests/similarity_reference.py bit-equal
to the reference, a pair of similarity_wj_small whose value changes in the last bit when i and j swap roles, and every file no
larger than the largest fixture already committed.

usage:  python tests/golden/make_golden_similarity.py
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for shim in ('_lightfm_shim', '_sksparse_shim', '_numba_shim'):
    sys.path.insert(0, os.path.join(HERE, shim))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
warnings.filterwarnings('ignore')

import numpy as np
import scipy.sparse as sps

from polara.lib import similarity as ref

import similarity_reference as res

MAX_BYTES = 415196          # the largest fixture committed before these (coffee_ml1m.npz)
N_WIDE, N_COLD, N_LABELS = 2597, 70, 600
REF_FUNCS = {
    'cosine': lambda F, fill: ref.cosine_similarity(F, fill_diagonal=fill),
    'cosine-binary': lambda F, fill: ref.cosine_similarity(F, fill_diagonal=fill, assume_binary=True),
    'tfidf-cosine': lambda F, fill: ref.cosine_tfidf_similarity(F, fill_diagonal=fill),
}


def wide_features(n_items, seed):
    """The feature CSR of the `wide` family over n_items items (the cases of the module docstring sit in the first 2 597)."""
    rng = np.random.RandomState(seed)
    rows = []
    clique = set(rng.choice(N_WIDE, 300, replace=False).tolist())
    empty = set(rng.choice(sorted(set(range(N_WIDE)) - clique), 5, replace=False).tolist())
    heavy = sorted(set(range(N_WIDE)) - clique - empty)[17]
    for i in range(n_items):
        if i in empty:
            labels = []
        elif i == heavy:
            labels = sorted(rng.choice(np.arange(1, N_LABELS), 130, replace=False).tolist())
        else:
            # 1-4 labels, mostly 1 or 2 (the product stays small enough to store whole)
            labels = sorted(rng.choice(np.arange(1, N_LABELS), rng.choice(4, p=[.7, .2, .07, .03]) + 1, replace=False).tolist())
            if i in clique:                                      # label 0 is the one 300 items carry, most of them alone:
                labels = [0] + (labels[:3] if rng.rand() < 0.1 else [])     # their 90 000 pairs then share a few values
        rows.append(labels)
    indptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int64)
    indices = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows if r] or [np.zeros(0, np.int32)]).astype(np.int32)
    data = np.where(rng.rand(len(indices)) < 0.2, rng.randint(2, 6, len(indices)), 1).astype(np.float64)
    for pos in rng.choice(np.flatnonzero(indices != 0), 2, replace=False):   # two explicitly stored zeros
        data[pos] = 0.0
    return sps.csr_matrix((data, indices, indptr), shape=(n_items, N_LABELS)), heavy


def weighted_features(n_items, n_labels, most, seed):
    rng = np.random.RandomState(seed)
    rows = [sorted(rng.choice(n_labels, rng.randint(1, most + 1), replace=False).tolist()) for _ in range(n_items)]
    rows[3] = []                                                    # one item without labels
    indptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int64)
    indices = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows if r]).astype(np.int32)
    data = rng.randint(1, 30, len(indices)) * 0.1                  # non-dyadic weights: sums depend on their order
    return sps.csr_matrix((data, indices, indptr), shape=(n_items, n_labels))


def put(out, key, S):
    out[key + '_indptr'] = S.indptr.astype(np.int64)
    out[key + '_indices'] = S.indices.astype(np.int32)
    out[key + '_data'] = S.data.astype(np.float64)
    out[key + '_shape'] = np.array(S.shape, np.int64)


def put_features(out, F, prefix='f'):
    put(out, prefix, F)


def check_cover(name, S, symmetric):
    S = res.canonical(S)
    assert np.isfinite(S.data).all(), name
    cols = S.indices
    for lo, hi in ((0, 512), (512, 1024), (1536, 2048), (2048, S.shape[1])):
        assert ((cols >= lo) & (cols < hi)).any(), '%s: no stored entry in columns [%d, %d)' % (name, lo, hi)
    if symmetric:
        assert res.same_bits(S, res.canonical(S.T)), name + ': not bitwise symmetric'


def save(name, out):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, '%s: %d bytes' % (name, size)
    print('%-28s %7d bytes' % (name, size))


def jaccard_counted(F, fill):
    """The contract of the Jaccard kind: the reference's own division on the fp64 intersection count."""
    F01 = (F != 0)
    nf = F01.getnnz(axis=1)
    S = F01.astype(np.float64).dot(F01.T)
    ref._jaccard_similarity_inplace(S.data, S.indices, S.indptr, nf)
    if fill:
        ref.set_diagonal_values(S, 1)
    return S


def wide():
    F_all, heavy = wide_features(N_WIDE + N_COLD, seed=101)
    F = F_all[:N_WIDE].tocsr()
    assert F.has_sorted_indices and (F.getnnz(axis=1) == 0).sum() == 5 and (F.data == 0).sum() == 2
    assert F[heavy].nnz == 130 and F.getnnz(axis=0)[0] == 300
    cross = {}
    put_features(cross, F_all[N_WIDE:].tocsr(), 'rows')
    for kind in res.KINDS:
        out = {'kind': np.str_(kind)}
        put_features(out, F)
        for fill in (False, True):
            key = 'fill%d' % fill
            if kind == 'jaccard':
                S = res.canonical(jaccard_counted(F.copy(), fill))
                run = res.canonical(ref.jaccard_similarity(F.copy(), fill_diagonal=fill))
                assert res.same_bits(res.jaccard(F, fill, counted=False), run), 'jaccard as run: restatement differs'
                assert np.array_equal(S.indptr, run.indptr) and np.array_equal(S.indices, run.indices)
                assert not np.array_equal(S.data, run.data), 'the boolean-product quirk is gone: the two Jaccards agree'
                out[key + '_data_as_run'] = run.data
            else:
                S = res.canonical(REF_FUNCS[kind](F.copy(), fill))
            check_cover('wide %s fill=%s' % (kind, fill), S, symmetric=True)
            assert res.same_bits(res.similarity(F, kind, fill), S), (kind, fill, 'restatement differs from the reference')
            put(out, key, S)
        save('similarity_wide_' + kind.replace('-', '_'), out)
        # the cross block: the reference's matrix over the stacked items
        full = jaccard_counted(F_all.copy(), True) if kind == 'jaccard' else REF_FUNCS[kind](F_all.copy(), True)
        block = res.canonical(full.tocsr()[N_WIDE:, :N_WIDE])
        check_cover('cross ' + kind, block, symmetric=False)
        assert res.same_bits(res.cross(F_all[N_WIDE:], F, kind), block), (kind, 'cross restatement differs')
        put(cross, kind, block)
    save('similarity_cross', cross)


def role_sensitive_pair(F):
    """A pair (i < j) of F whose weighted Jaccard value changes when i and j swap roles, or None."""
    _, rows = res._rows(F)
    for i in range(F.shape[0]):
        for j in range(i + 1, F.shape[0]):
            mn, mx = res.weighted_pair(rows[i], rows[j])
            mn2, mx2 = res.weighted_pair(rows[j], rows[i])
            if mn and mn / mx != mn2 / mx2:
                return i, j
    return None


def without_stored_zeros(S, fill, F):
    """The reference's weighted Jaccard matrix, canonical.  With fill_diagonal=False the reference ends in
    `setdiag(sign(S.diagonal()))`, and SciPy's setdiag with an array STORES the 0.0 of an item without labels; the contract
    here is that such a diagonal is not stored, so exactly those explicit zeros are dropped (asserted: nothing else is)."""
    S = res.canonical(S)
    zeros = int((S.data == 0).sum())
    assert zeros == (0 if fill else int((F.getnnz(axis=1) == 0).sum())), 'unexpected stored zeros: %d' % zeros
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    assert (rows[S.data == 0] == S.indices[S.data == 0]).all()
    S.eliminate_zeros()
    return S


def weighted():
    F = weighted_features(2100, 700, 3, seed=202)
    for fill, name in ((True, 'similarity_wj'), (False, 'similarity_wj_nofill')):
        S = without_stored_zeros(ref.jaccard_similarity_weighted(F.copy(), fill_diagonal=fill), fill, F)
        check_cover(name, S, symmetric=True)
        assert res.same_bits(res.jaccard_weighted(F, fill), S), name + ': restatement differs from the reference'
        out = {'fill_diagonal': np.bool_(fill), 'n_cross_rows': np.int64(60)}
        put_features(out, F)
        put(out, 'S', S)
        save(name, out)
    n_cols = 2100 - 60
    block = res.canonical(S[n_cols:, :n_cols])
    assert block.nnz > 0 and res.same_bits(res.cross(F[n_cols:], F[:n_cols], 'jaccard-weighted'), block), 'wj cross block'

    for seed in range(300, 340):
        Fs = weighted_features(150, 40, 5, seed=seed)
        pair = role_sensitive_pair(Fs)
        if pair is not None:
            break
        print('similarity_wj_small: seed %d has no role-sensitive pair' % seed)
    out = {'role_pair': np.array(pair if pair is not None else (-1, -1), np.int64)}
    put_features(out, Fs)
    for fill in (False, True):
        S = without_stored_zeros(ref.jaccard_similarity_weighted(Fs.copy(), fill_diagonal=fill), fill, Fs)
        assert np.isfinite(S.data).all() and res.same_bits(S, res.canonical(S.T))
        assert res.same_bits(res.jaccard_weighted(Fs, fill), S), 'wj_small: restatement differs from the reference'
        put(out, 'fill%d' % fill, S)
    if pair is None:        # no seed gave one: then the device rule (i = min, j = max) must equal the reference on every pair
        print('similarity_wj_small: no role-sensitive pair found; the rule was checked on every pair instead')
    save('similarity_wj_small', out)


if __name__ == '__main__':
    wide()
    weighted()
