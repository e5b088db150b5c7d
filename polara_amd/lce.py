"""Local Collective Embeddings (polara/recommender/hybrid/models.py:120-225, coldstart/models.py:122-146,
lib/optimize.py:309-391): a non-negative factorisation of the item x label matrix Xs ~ W Hs and the item x user matrix
Xu ~ W Hu with one shared item factor W, regularised by a kNN graph of the items, by multiplicative updates.

The solver keeps all three factors on the device as tall row-major fp64 blocks — W [n_items x k], HsT [n_labels x k],
HuT [n_users x k]; the H factors transposed, which is what the sparse products, `gram` and `tsmm` take — and a pass is
three fused updates (csrc/lce.hip), five sparse products, three Gram products and one reduction of the objective.  One
double, the objective, visits the host per pass.  Single process."""
import math
from timeit import default_timer as timer

import numpy as np

from . import scoring
from .coldstart import (ItemColdStartEvaluationMixin, ItemColdStartRecommenderMixin, ItemColdStartSVDModelMixin,
                        _frame_data, check_image_memory, stack_features)
from .factor_serving import FactorQueriesMixin
from .models import RecommenderModel

FLOOR = 1e-10           # the reference's np.maximum(., 1e-10) under every division


def solver_bytes(n_items, n_labels, n_users, k, nnz_s, nnz_u, nnz_a, fused_max_rank=128):
    """Device bytes a build takes (upper estimate): a factor and its numerator block per side (fp64), the product block
    of the composed update above the fused rank, and per stored entry the transposed image (row ids, fp64 values) and
    the scaled fp64 values of the three sparse matrices."""
    rows = 2 * (int(n_items) + int(n_labels) + int(n_users))
    if int(k) > fused_max_rank:
        rows += max(int(n_items), int(n_labels), int(n_users))
    return 8 * int(k) * rows + (12 + 8) * (int(nnz_s) + int(nnz_u)) + 8 * int(nnz_a)


def check_solver_memory(n_items, n_labels, n_users, k, nnz_s, nnz_u, nnz_a, free_bytes, fused_max_rank=128):
    """The guard of the build (like coldstart.check_image_memory): it must fit in half of the free device memory."""
    need = solver_bytes(n_items, n_labels, n_users, k, nnz_s, nnz_u, nnz_a, fused_max_rank)
    if need > free_bytes / 2:
        raise MemoryError('LCE: a rank-%d build over %d items, %d labels and %d users needs %d bytes (%.2f GB) on the device, '
                          'more than half of the %.2f GB of free device memory'
                          % (k, n_items, n_labels, n_users, need, need / 1e9, free_bytes / 1e9))
    return need


def initial_factors(n_items, n_labels, n_users, k, seed=None):
    """(W [n x k], Hs [k x v1], Hu [k x v2]) drawn like optimize.py:323-326: in that order and those shapes from
    `RandomState(seed)`, or from NumPy's global generator when seed is None."""
    random = np.random if seed is None else np.random.RandomState(seed)
    W = random.rand(n_items, k)
    Hs = random.rand(k, n_labels)
    Hu = random.rand(k, n_users)
    return W, Hs, Hu


def _device_csr(ops, M):
    if hasattr(M, 'tocsr'):                 # a SciPy matrix
        M = M.tocsr()
        M.sort_indices()
        return ops.csr(M.indptr, M.indices, np.asarray(M.data, dtype=np.float64), M.shape)
    return M


def local_collective_embeddings(ops, Xs, Xu, A, k, alpha=0.1, beta=0.05, lamb=1, epsilon=1e-4, maxiter=15, seed=None,
                                init=None, verbose=False, stats=None, comm=None, fused=None):
    """optimize.py:309-391 on the device.  Xs [n_items x n_labels], Xu [n_items x n_users], A [n_items x n_items] (the item
    graph): ops-level CSR matrices or SciPy ones.  Returns the DEVICE blocks (W [n_items x k], HuT [n_users x k],
    HsT [n_labels x k]).  init = (W, Hs, Hu) host arrays in the reference's shapes instead of the seeded draw; `stats`
    (a dict) receives the objective history and the pass count; `fused`: see HipOps.lce_update (None: by rank).
    Pass `p` runs, from the second on, the stopping rule of optimize.py:382-387: stop when p > maxiter or the objective
    moved by less than epsilon — maxiter = 15 is 16 passes."""
    if comm is not None and getattr(comm, 'world', 1) > 1:
        raise NotImplementedError('LCE: multi-process builds are not supported (comm.world = %d)' % comm.world)
    Xs, Xu, A = (_device_csr(ops, M) for M in (Xs, Xu, A))
    n, v1 = (int(x) for x in Xs.shape)
    v2 = int(Xu.shape[1])
    k = int(k)
    if int(Xu.shape[0]) != n or tuple(int(x) for x in A.shape) != (n, n):
        raise ValueError('LCE: Xs %s, Xu %s and the item graph %s do not describe the same items'
                         % (tuple(Xs.shape), tuple(Xu.shape), tuple(A.shape)))
    if k < 1:
        raise ValueError('LCE: rank %d' % k)
    if hasattr(ops, 'free_bytes'):
        check_solver_memory(n, v1, v2, k, Xs.nnz, Xu.nnz, A.nnz, ops.free_bytes(), ops.lce_fused_max_rank())
    if init is None:
        init = initial_factors(n, v1, v2, k, seed)
    W0, Hs0, Hu0 = (np.asarray(a, dtype=np.float64) for a in init)
    if W0.shape != (n, k) or Hs0.shape != (k, v1) or Hu0.shape != (k, v2):
        raise ValueError('LCE: initial factors of shapes %s, %s, %s for (%d x %d), (%d x %d), (%d x %d)'
                         % (W0.shape, Hs0.shape, Hu0.shape, n, k, k, v1, k, v2))
    alpha, beta, lamb = float(alpha), float(beta), float(lamb)
    gamma = 1. - alpha
    W = ops.to_device(np.ascontiguousarray(W0))
    HsT = ops.to_device(np.ascontiguousarray(Hs0.T))
    HuT = ops.to_device(np.ascontiguousarray(Hu0.T))
    XsT, XuT = Xs.T, Xu.T                                   # device transposes (pk_csr_transpose), cached on the matrices
    # the scalars of the W update ride on the stored values: alpha Xs, gamma Xu, beta A (fp64 copies of the values)
    Xs_a, Xu_g, A_b = ops.csr_scaled(Xs, alpha), ops.csr_scaled(Xu, gamma), ops.csr_scaled(A, beta)
    ones = ops.to_device(np.ones((n, 1)))
    c = ops.spmm(ops.csr_scaled(A.T, beta), ones).reshape(-1).contiguous()      # beta d, d = the column sums of A
    # alpha ||Xs||^2 + gamma ||Xu||^2 from the scaled values: sum (alpha x)^2 / alpha
    vs, vu = ops.csr_values(Xs_a).reshape(-1, 1), ops.csr_values(Xu_g).reshape(-1, 1)
    pairs = [(1. / s, v, v, None) for s, v in ((alpha, vs), (gamma, vu)) if s != 0. and v.numel()]
    const = float(ops.lce_dots(pairs)[0].item()) if pairs else 0.
    Ns, Nu, BAW = ops.empty(v1, k), ops.empty(v2, k), ops.empty(n, k)

    def products():
        """what the next pass and the objective read of the new W: W^T W, Xs^T W, Xu^T W, beta A W"""
        ops.spmm(XsT, W, out=Ns)
        ops.spmm(XuT, W, out=Nu)
        ops.spmm(A_b, W, out=BAW)
        return ops.gram(W)

    G_W = products()
    history = []
    it = 1
    while True:
        ops.lce_update(HsT, Ns, G_W, ma=alpha, a=alpha, lamb=lamb, fused=fused)               # optimize.py:350-352
        ops.lce_update(HuT, Nu, G_W, ma=gamma, a=gamma, lamb=lamb, fused=fused)               # optimize.py:354-356
        G_s, G_u = ops.gram(HsT), ops.gram(HuT)
        # numerator of W, accumulated on beta A W: + alpha Xs Hs^T + gamma Xu Hu^T                   optimize.py:359
        ops.spmm_acc(Xs_a, HsT, BAW)
        ops.spmm_acc(Xu_g, HuT, BAW)
        ops.lce_update(W, BAW, G_s, ma=alpha, M2=G_u, mb=gamma, a=1., lamb=lamb, c=c, fused=fused)   # optimize.py:360-363
        G_W = products()
        diag = lambda G: G.diagonal().unsqueeze(1)
        obj = ops.lce_dots([(-2. * alpha, HsT, Ns, None), (alpha, G_W, G_s, None),                   # optimize.py:374
                            (-2. * gamma, HuT, Nu, None), (gamma, G_W, G_u, None),                   # :375
                            (1., W, W, c), (-1., W, BAW, None),                                      # :376
                            (lamb, diag(G_W), None, None), (lamb, diag(G_s), None, None), (lamb, diag(G_u), None, None)],
                           bias=const)
        history.append(float(obj[0].item()))                # the pass's one host read
        if it > 1:
            delta = abs(history[-1] - history[-2])
            if verbose:
                print('Iteration: ', it, 'Objective: ', history[-1], 'Delta: ', delta)
            if it > maxiter or delta < epsilon:
                break
        it += 1
    if stats is not None:
        stats.update(objective=history, passes=len(history))
    return W, HuT, HsT


class LCEModel(FactorQueriesMixin, RecommenderModel):
    """hybrid/models.py:120-225.  `factors` holds host arrays like everywhere else — users [n_users x k], items
    [n_items x k], f'{itemid}_features' [n_labels x k] — and the device copies of the user and feature factors stay for
    the passes.  A rank change invalidates the model: LCE factors are not nested, there is no truncation.
    The item graph is built on the host with scikit-learn exactly as the reference does, or given as `item_graph`
    (a SciPy matrix [n_items x n_items])."""

    def __init__(self, *args, item_features=None, **kwargs):
        super().__init__(*args, **kwargs)
        self._rank = 10
        self.factors = {}
        self.alpha = 0.1
        self.beta = 0.05
        self.max_neighbours = 10
        self.item_features = item_features if item_features is not None else getattr(self.data, 'item_features', None)
        self.binary_features = True
        self.item_features_labels = None
        self.item_graph = None
        self.seed = None
        self.show_error = False
        self.regularization = 1
        self.max_iterations = 15
        self.tolerance = 0.0001
        self.method = 'LCE'
        self.build_stats = {}
        self.graph_time = []
        self._factors_dev = None            # (host user factors of `factors`, HuT and HsT on the device) of the last build
        self.data.subscribe(self.data.on_change_event, self._clean_metadata)

    def _clean_metadata(self):
        super()._clean_metadata()
        self.item_features_labels = None

    def encode_item_features(self):
        """The one-hot matrix of the (training) items in the model's item order [n_items x n_labels] (SciPy CSR); a data
        object without a cold-start split has one item index (hybrid/models.py:155-170)."""
        d = self.data
        if _frame_data(d):
            index = d.index.itemid
            index = getattr(index, 'training', index)
            frame = self.item_features.reindex(index.old.values, fill_value=[])
            one_hot, self.item_features_labels = stack_features(frame)
            return one_hot
        return ItemColdStartSVDModelMixin.encode_item_features(self)

    def build_item_graph(self, item_features, n_neighbors):
        """hybrid/models.py:173-182: the directed kNN graph of the items, 1 + n_neighbors entries per row (the item itself
        included): ones for binary features, distances otherwise."""
        try:
            from sklearn.neighbors import NearestNeighbors
        except ImportError:
            raise NotImplementedError('Install scikit-learn to construct graph for LCE model.')
        nbrs = NearestNeighbors(n_neighbors=1 + n_neighbors).fit(item_features)
        if self.binary_features:
            return nbrs.kneighbors_graph(item_features)
        return nbrs.kneighbors_graph(item_features, mode='distance')

    def _item_graph(self, one_hot):
        n_items = one_hot.shape[0]
        if self.item_graph is not None:
            A = self.item_graph
            if not hasattr(A, 'tocsr') or tuple(A.shape) != (n_items, n_items):
                raise ValueError('item_graph must be a SciPy sparse matrix of shape (%d, %d), got %s'
                                 % (n_items, n_items, getattr(A, 'shape', type(A).__name__)))
            return A.tocsr()
        start = timer()
        A = self.build_item_graph(one_hot, min(self.max_neighbours, int(math.sqrt(n_items)))).tocsr()
        self.graph_time.append(timer() - start)
        return A

    def build(self):
        self._require_single_process_build()
        if self.item_features is None:
            raise ValueError('%s needs item features: pass item_features= or use a data object that has them' % self.method)
        ops = self.ops
        one_hot = self.encode_item_features()                   # Xs: item x label, ones (stack_features(normalize=False))
        graph = self._item_graph(one_hot)
        train = self._training_device_csr()                     # Xu^T
        if train.shape[1] != one_hot.shape[0]:
            raise ValueError('features for %d items, the training matrix has %d' % (one_hot.shape[0], train.shape[1]))
        start = timer()
        stats = {}
        W, HuT, HsT = local_collective_embeddings(ops, one_hot, train.T, graph, k=self.rank, alpha=self.alpha, beta=self.beta,
                                                  lamb=self.regularization, epsilon=self.tolerance,
                                                  maxiter=self.max_iterations, seed=self.seed, verbose=self.show_error,
                                                  stats=stats)
        ops.synchronize()
        self._track(start)
        self.build_stats = stats
        self._set_factors(HuT, W, kept=(HsT,), features=HsT)

    def _extra_factors_device(self):
        HsT = self.factors[f'{self.data.fields.itemid}_features']
        return (self.ops.to_device(np.ascontiguousarray(HsT, dtype=np.float64)),)


class LCEModelItemColdStart(ItemColdStartEvaluationMixin, ItemColdStartRecommenderMixin, LCEModel):
    """coldstart/models.py:122-146: a cold item with the one-hot feature row x scores user u with
    max(x Hs^T pinv(Hs Hs^T), 0) . Hu[:, u].  The queries are the cold items, the catalogue the rows of HuT in
    descending-norm order, nothing is masked (scoring.recommend_dense).  The reference reads
    `factors['item_features']`, so its model only runs when the item column is called `item`; the key here is
    f'{itemid}_features' like in the rest of the package.  Like the reference's, the lists range over ALL training users
    whether the data names representative users or not (only MP(cs) restricts itself to them)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.method = 'LCE(cs)'
        self.item_features_invgram = None
        self._user_image = None             # (host user factors, FactorImage of HuT by norm, host order: position -> user)
        self._features_dev = None           # (host invgram, HsT and invgram on the device)
        self._cold_dev = None
        self.data.subscribe(self.data.on_update_event, self._clean_cold_items)

    def _clean_metadata(self):
        super()._clean_metadata()
        self._user_image = self._features_dev = self._cold_dev = None

    def _clean_cold_items(self):
        self._cold_dev = None

    _cold_one_hot = ItemColdStartSVDModelMixin._cold_one_hot
    _cold_features_device = ItemColdStartSVDModelMixin._cold_features_device

    def build(self, *args, **kwargs):
        super().build(*args, **kwargs)
        HsT = self.factors[f'{self.data.fields.itemid}_features']
        # (Hs Hs^T)^+ on the host in fp64 with NumPy's default cut-off: k x k, part of the contract
        self.item_features_invgram = np.linalg.pinv(HsT.T @ HsT)
        self._cold_dev = None
        self._user_factors_device()

    def _user_factors_device(self):
        """(FactorImage of HuT by descending row norm, host int64 order: catalogue position -> training user)"""
        Hu = self.factors.get(self.data.fields.userid, None)
        if Hu is None:
            raise ValueError('%s: no user factors (build the model first)' % self.method)
        cached = self._user_image
        if cached is not None and cached[0] is Hu:
            return cached[1], cached[2]
        ops = self.ops
        if hasattr(ops, 'free_bytes'):
            check_image_memory(Hu.shape[0], Hu.shape[1], ops.free_bytes())
        order, Xs = self._rows_by_norm(self._user_factors_block())
        image = scoring.FactorImage(ops, Xs)
        self._user_image = (Hu, image, order)
        return image, order

    def _cold_queries_device(self):
        """E = max((F_cold HsT) invgram, 0) on the device (coldstart/models.py:143-144)"""
        G = self.item_features_invgram
        if G is None:
            raise ValueError('%s: no feature embeddings (build the model first)' % self.method)
        ops = self.ops
        self._user_factors_block()
        HsT = self._factors_dev[2]
        cached = self._features_dev
        if cached is None or cached[0] is not G:
            cached = self._features_dev = (G, ops.to_device(np.ascontiguousarray(G, dtype=np.float64)))
        F = self._cold_features_device()
        if F.shape[1] != HsT.shape[0]:
            raise ValueError('cold item features over %d labels, the embeddings over %d' % (F.shape[1], HsT.shape[0]))
        return ops.clamp_min(ops.coldstart_queries(F, HsT, cached[1]), 0.0)
