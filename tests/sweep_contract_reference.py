"""The contract of ONE candidate sweep (csrc/score.hip), restated in NumPy on fp64 inputs: what the raw lists a sweep leaves
must satisfy for the certification of the re-scoring kernel (csrc/rescore.hip) to stand.  No device, no library.

A sweep leaves, per user, one list of KC (score float32, item int32) entries for every set of tiles that was swept on its
own: one list for a single sweep or a merged two-phase sweep (all tiles), S lists for S item splits (split h owns the tiles
h, h + S, ...).  With U = the items of the list's tiles that the user has not seen (all of them without a seen filter),

    rel  = 3 * 2^-16 + (4 K + 10) * 2^-23            (the error model in the header of score.hip, `bound` of rescore.hip)
    b(i) = rel * ||E_u|| * ||V_i||

the conditions are

  C1, ids.          entries with id >= 0 are distinct, lie in U and are < n_items; negative ids only behind the valid ones
  C2, scores.       |score - E_u . V_i| <= b(i) for every valid entry
  C3, completeness. a list that holds a negative id holds every item of U; otherwise, with kth = min(score), every item of
                    U that is not in the list has  E_u . V_i <= kth + 2 * max_i b(i) + |kth| * 2^-15  (the 2^-15 is the
                    key-sort tolerance stated in the header of score.hip)

for EVERY user u < n_users and every list: the checker leaves nobody and nothing out (an all-zero row of E satisfies the
three conditions trivially; the padding users of the last group are never read)."""
import numpy as np

TILE = 32
KEY_SORT_TOL = 2.0 ** -15


class ContractViolation(AssertionError):
    """`condition` is 'C1', 'C2' or 'C3'"""

    def __init__(self, condition, message):
        super().__init__('%s: %s' % (condition, message))
        self.condition = condition


def sweep_rel_error(K):
    return 3 * 2.0 ** -16 + (4 * K + 10) * 2.0 ** -23


def n_tiles_of(n_items):
    return -(-n_items // TILE)


def all_tiles(n_items):
    return np.arange(n_tiles_of(n_items))


def split_tiles(n_items, h, S, base=0):
    """the tiles split h of S owns: base + h, base + h + S, ..."""
    return np.arange(base + h, n_tiles_of(n_items), S)


class SweepContract:
    """V [n_items x K], E [n_users x K] in fp64; seen = (indptr, indices) of the users' seen items or None.  The exact scores,
    the bounds and the seen mask are computed once and shared by every `check`."""

    def __init__(self, V, E, seen=None):
        V, E = np.asarray(V, dtype=np.float64), np.asarray(E, dtype=np.float64)
        self.n_items, self.K = V.shape
        self.n_users = E.shape[0]
        self.exact = E @ V.T
        self.rel = sweep_rel_error(self.K)
        self.bound = self.rel * np.linalg.norm(E, axis=1)[:, None] * np.linalg.norm(V, axis=1)[None, :]
        self.bound_max = self.bound.max(axis=1)
        self.seen_mask = np.zeros((self.n_users, self.n_items), dtype=bool)
        if seen is not None:
            indptr, indices = seen
            for u in range(self.n_users):
                self.seen_mask[u, indices[indptr[u]:indptr[u + 1]]] = True
        self.tile_of = np.arange(self.n_items) // TILE

    def without_filter(self):
        """the same inputs with no seen filter (shares the exact scores)"""
        other = object.__new__(SweepContract)
        other.__dict__.update(self.__dict__)
        other.seen_mask = np.zeros_like(self.seen_mask)
        return other

    def universe(self, tiles):
        """bool [n_users x n_items]: U of a list that owns `tiles`"""
        owned = np.zeros(n_tiles_of(self.n_items), dtype=bool)
        owned[np.asarray(tiles, dtype=np.int64)] = True
        return owned[self.tile_of][None, :] & ~self.seen_mask

    def check(self, KC, cs, ci, tiles, completeness=True):
        """cs float32, ci int32 as [lists][n_pad][KC] (n_pad >= n_users); tiles: per list, the tiles it owns.  Raises
        ContractViolation under the first condition that fails; returns the worst |error| / b over all valid entries (0 when
        there is none with b > 0).  completeness=False: C1 and C2 only — for the raw lists of a two-phase sweep, whose
        splits start from the head's thresholds and keep only what beats them (the merged list is the one C3 holds for)."""
        cs, ci = np.asarray(cs), np.asarray(ci)
        assert cs.dtype == np.float32 and ci.dtype == np.int32 and cs.shape == ci.shape and cs.ndim == 3, (cs.dtype, ci.dtype, cs.shape)
        assert cs.shape[0] == len(tiles) and cs.shape[1] >= self.n_users and cs.shape[2] == KC, (cs.shape, len(tiles), KC)
        worst = 0.0
        n = self.n_users
        rows = np.arange(n)[:, None]
        for l in range(cs.shape[0]):
            s, i = cs[l, :n].astype(np.float64), ci[l, :n].astype(np.int64)
            U = self.universe(tiles[l])
            valid = i >= 0
            # ---- C1
            if (i[valid] >= self.n_items).any():
                u, t = np.argwhere(valid & (i >= self.n_items))[0]
                raise ContractViolation('C1', 'list %d user %d slot %d: item %d of %d' % (l, u, t, i[u, t], self.n_items))
            behind = valid[:, 1:] & ~valid[:, :-1]
            if behind.any():
                u, t = np.argwhere(behind)[0]
                raise ContractViolation('C1', 'list %d user %d: a valid entry in slot %d behind an empty one' % (l, u, t + 1))
            safe = np.where(valid, i, 0)
            in_U = U[rows, safe]
            if (valid & ~in_U).any():
                u, t = np.argwhere(valid & ~in_U)[0]
                why = 'seen by the user' if self.seen_mask[u, i[u, t]] else 'of a tile the list does not own'
                raise ContractViolation('C1', 'list %d user %d slot %d: item %d is %s' % (l, u, t, i[u, t], why))
            held = np.zeros((n, self.n_items), dtype=np.int64)
            np.add.at(held, (np.broadcast_to(rows, i.shape)[valid], i[valid]), 1)
            if (held > 1).any():
                u, j = np.argwhere(held > 1)[0]
                raise ContractViolation('C1', 'list %d user %d: item %d appears %d times' % (l, u, j, held[u, j]))
            # ---- C2
            err = np.abs(s - self.exact[rows, safe])
            lim = self.bound[rows, safe]
            bad = valid & ~(err <= lim)         # (a NaN score fails)
            if bad.any():
                u, t = np.argwhere(bad)[0]
                raise ContractViolation('C2', 'list %d user %d slot %d item %d: score %r, exact %r, |error| %.3e > b %.3e'
                                        % (l, u, t, i[u, t], cs[l, u, t], self.exact[u, i[u, t]], err[u, t], lim[u, t]))
            with np.errstate(invalid='ignore', divide='ignore'):
                ratio = np.where(valid & (lim > 0), err / lim, 0.0)
            worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
            # ---- C3
            if not completeness:
                continue
            held = held.astype(bool)
            left_out = U & ~held
            short = ~valid.all(axis=1)
            if (short & left_out.any(axis=1)).any():
                u = int(np.flatnonzero(short & left_out.any(axis=1))[0])
                raise ContractViolation('C3', 'list %d user %d: %d of %d slots filled although %d items are eligible (last id %d)'
                                        % (l, u, valid[u].sum(), KC, U[u].sum(), i[u, -1]))
            full = ~short
            kth = np.where(full, s.min(axis=1), np.inf)
            slack = 2 * self.bound_max + np.abs(np.where(full, kth, 0.0)) * KEY_SORT_TOL
            best_out = np.where(left_out, self.exact, -np.inf).max(axis=1)
            over = full & ~(best_out <= kth + slack)
            if over.any():
                u = int(np.flatnonzero(over)[0])
                j = int(np.argmax(np.where(left_out[u], self.exact[u], -np.inf)))
                raise ContractViolation('C3', 'list %d user %d: item %d is left out with exact score %r > kth %r + slack %.3e'
                                        % (l, u, j, self.exact[u, j], kth[u], slack[u]))
        return worst

    def exact_lists(self, KC, tiles, n_pad=None):
        """the lists an error-free sweep would leave: per list the KC best of U by (exact score descending, item ascending),
        scores rounded to float32, empty slots (-inf, -1)"""
        n_pad = n_pad or -(-self.n_users // TILE) * TILE
        cs = np.full((len(tiles), n_pad, KC), -np.inf, dtype=np.float32)
        ci = np.full((len(tiles), n_pad, KC), -1, dtype=np.int32)
        for l, tl in enumerate(tiles):
            U = self.universe(tl)
            for u in range(self.n_users):
                s = np.where(U[u], self.exact[u], -np.inf)
                order = np.lexsort((np.arange(self.n_items), -s))[:KC]
                order = order[U[u][order]]
                cs[l, u, :len(order)] = s[order]
                ci[l, u, :len(order)] = order
        return cs, ci


def merged_best(KC, ws, wi, n_users):
    """what merge_candidates_kernel documents: per user the KC best float32 entries of the union of the raw lists
    ws, wi [lists][n_pad][KC] by (score descending, item ascending), as (scores, ids) [n_users][KC]; empty slots (-inf, -1)"""
    out_s = np.full((n_users, KC), -np.inf, dtype=np.float32)
    out_i = np.full((n_users, KC), -1, dtype=np.int32)
    for u in range(n_users):
        s, i = ws[:, u, :].ravel(), wi[:, u, :].ravel()
        keep = i >= 0
        s, i = s[keep], i[keep]
        order = np.lexsort((i, -s.astype(np.float64)))[:KC]
        out_s[u, :len(order)] = s[order]
        out_i[u, :len(order)] = i[order]
    return out_s, out_i
