"""The similarity restatement of tests/similarity_reference.py next to the imported reference (`polara.lib.similarity`, through
the test-only numba stand-in of tests/golden) on fresh seeds: values, pattern and format after canonicalisation.  No GPU.
Skips where the reference is not on this machine.  Runs in a child process, like tests/test_dropin_sim.py (the stand-ins
must not leak into the other tests)."""
import json
import os
import subprocess
import sys

import pytest

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'polara')), reason='the reference is not on this machine')

CHILD = r'''
import json, os, sys, warnings
here, ref_root = sys.argv[1], sys.argv[2]
sys.path[:0] = [os.path.join(here, 'golden', '_numba_shim'), ref_root, here]
warnings.filterwarnings('ignore')
import numpy as np
import scipy.sparse as sps
from polara.lib import similarity as ref
import similarity_reference as res

def features(n, n_labels, most, seed, weights):
    rng = np.random.RandomState(seed)
    rows = [sorted(rng.choice(n_labels, rng.randint(0, most + 1), replace=False).tolist()) for _ in range(n)]
    indptr = np.r_[0, np.cumsum([len(r) for r in rows])]
    indices = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows])
    data = rng.randint(1, 30, len(indices)) * 0.1 if weights else np.ones(len(indices))
    return sps.csr_matrix((data, indices, indptr), shape=(n, n_labels))

out = {}
for seed in (11, 12, 13):
    F = features(400, 60, 4, seed, weights=seed != 12)
    for fill in (False, True):
        pairs = {
            'cosine': (ref.cosine_similarity(F.copy(), fill_diagonal=fill), res.similarity(F, 'cosine', fill)),
            'cosine-binary': (ref.cosine_similarity(F.copy(), fill_diagonal=fill, assume_binary=True),
                              res.similarity(F, 'cosine-binary', fill)),
            'tfidf-cosine': (ref.cosine_tfidf_similarity(F.copy(), fill_diagonal=fill), res.similarity(F, 'tfidf-cosine', fill)),
            'jaccard as run': (ref.jaccard_similarity(F.copy(), fill_diagonal=fill), res.jaccard(F, fill, counted=False)),
        }
        for kind, (theirs, ours) in pairs.items():
            out['%s seed %d fill %d' % (kind, seed, fill)] = bool(res.same_bits(res.canonical(theirs), ours))
    G = features(90, 25, 5, seed + 100, weights=True)
    for fill in (False, True):
        theirs = res.canonical(ref.jaccard_similarity_weighted(G.copy(), fill_diagonal=fill))
        theirs.eliminate_zeros()          # the 0.0 the reference's setdiag stores on the diagonal of an item without labels
        ours = res.similarity(G, 'jaccard-weighted', fill)
        out['jaccard-weighted seed %d fill %d' % (seed, fill)] = bool(res.same_bits(theirs, ours) and ours.format == 'csr')
print('RESULT ' + json.dumps(out))
'''


def test_restatement_equals_the_imported_reference_on_fresh_seeds():
    r = subprocess.run([sys.executable, '-c', CHILD, HERE, REF], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1]
    out = json.loads(line[len('RESULT '):])
    assert len(out) == 3 * 2 * 5
    assert [k for k, ok in out.items() if not ok] == []
