"""Reference for collect(DISTINCT b) over remapped ids (the yardstick, not the code under test): the lists of
varlen_collect_ref.reach_lists on the dense ids, every element and every start mapped through `ids` (dense index ->
original id) and each list sorted again as Python ints -- ``sorted(ids[x] for x in list)`` -- so the order is the
signed order of the original ids, whatever order `ids` has."""
import numpy as np

from varlen_collect_ref import reach_lists


def mapped_lists(n, src, dst, a_mask, b_mask, lower, upper, ids):
    """({original id of a: sorted list of the original ids of D(a)}, the sorted list of their union); src / dst are
    dense ids relative to the window [0, n), ids[d] the original id of dense id d."""
    lists, union = reach_lists(n, src, dst, a_mask, b_mask, lower, upper)
    ids = [int(x) for x in ids]
    return ({ids[a]: sorted(ids[x] for x in v) for a, v in lists.items()}, sorted(ids[x] for x in union))


def id_sets():
    """name -> f(rng, n): n distinct original ids in dense order, the permutations the tests walk."""
    def identity(rng, n):
        return np.arange(n, dtype=np.int64)

    def reverse(rng, n):
        return np.arange(n, dtype=np.int64)[::-1].copy()

    def random(rng, n):
        return rng.permutation(n).astype(np.int64)

    def signed(rng, n):
        """negative ids, small ones, and ids near 2^40 and 2^62 mixed: only the signed order sorts them"""
        pools = [np.arange(-n, 0, dtype=np.int64) * 7 - 1, np.arange(n, dtype=np.int64) * 3,
                 (1 << 40) + np.arange(n, dtype=np.int64) * 5, (1 << 62) + np.arange(n, dtype=np.int64) * 11,
                 -(1 << 62) - np.arange(n, dtype=np.int64) * 13]
        pick = rng.integers(0, len(pools), n)
        out = np.array([pools[p][i] for i, p in enumerate(pick)], dtype=np.int64)
        assert len(set(out.tolist())) == n
        return out[rng.permutation(n)]

    return {"identity": identity, "reverse": reverse, "random": random, "signed": signed}
