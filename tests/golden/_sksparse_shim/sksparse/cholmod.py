"""cholesky(A, beta) -> Factor with CHOLMOD's conventions: P A' P^T = L L^T (A' = A + beta I), apply_P(b) = b[P],
apply_Pt the inverse, solve_Lt(y) = L^-T y.  Dense NumPy underneath; the permutation is seeded (PERMUTATION_SEED;
None: the identity)."""
import numpy as np
import scipy.linalg
import scipy.sparse as sps

PERMUTATION_SEED = 12345


class CholmodNotPositiveDefiniteError(np.linalg.LinAlgError):
    pass


class Factor:
    def __init__(self, A, beta=0.0):
        n = A.shape[0]
        self._P = (np.arange(n) if PERMUTATION_SEED is None
                   else np.random.RandomState(PERMUTATION_SEED).permutation(n))
        self.cholesky_inplace(A, beta)

    def cholesky_inplace(self, A, beta=0.0):
        K = (A.toarray() if sps.issparse(A) else np.asarray(A, dtype=np.float64)) + beta * np.eye(A.shape[0])
        K = np.tril(K) + np.tril(K, -1).T                 # the lower triangle is what CHOLMOD reads
        try:
            self._L = np.linalg.cholesky(K[np.ix_(self._P, self._P)])
        except np.linalg.LinAlgError as exc:
            raise CholmodNotPositiveDefiniteError(str(exc)) from None

    def P(self):
        return self._P

    def L(self):
        return sps.csc_matrix(self._L)

    def apply_P(self, b):
        return np.asarray(b)[self._P]

    def apply_Pt(self, b):
        out = np.empty_like(np.asarray(b))
        out[self._P] = b
        return out

    def solve_Lt(self, y, use_LDLt_decomposition=True):
        if use_LDLt_decomposition:
            raise NotImplementedError('the stand-in holds an LL^T factor only')
        return scipy.linalg.solve_triangular(self._L, np.asarray(y, dtype=np.float64), lower=True, trans='T')


def cholesky(A, beta=0, mode='auto', ordering_method='default', use_long=None):
    return Factor(A, beta)
