"""Test-only stand-in for scikit-sparse (not installed here): just enough of `sksparse.cholmod` for the reference's
HybridSVD (polara/recommender/hybrid/models.py, polara/lib/cholesky.py) to run when the golden fixtures are made.  The
factor is a dense NumPy Cholesky factor taken under a seeded NON-identity permutation, so the fixtures exercise the
invariance of the model under the choice of square root."""
__version__ = '0.4.8'
