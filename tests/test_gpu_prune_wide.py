"""k_prune<false> against oracle.robust_prune and knn_ref.prune_trace, through
pm_robust_prune_wide, at rows of 257, 960 and 1,024 dimensions: by the kernel's
own LDS sort and in the presorted form of hub lists; and the narrow routing."""
import numpy as np
import pytest

from tests import knn_wide_ref as W

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("presorted", [False, True], ids=["lds_sort", "presorted"])
DIMS = pytest.mark.parametrize("dim", [257, 960, 1024])


def check(ctx, oracle, X, verts, lists, m, alpha, presorted, expect_err=()):
    """Every list's result equals the oracle's; the lists in expect_err (above
    the LDS sort's limit, unsorted form) give length 0 and raise the flag."""
    import pacmann_amd as pm
    got, err = pm.robust_prune_wide(X, verts, lists, m, alpha, presorted, ctx)
    assert err == (1 if len(expect_err) else 0)
    for b, (u, lst) in enumerate(zip(verts, lists)):
        if b in expect_err:
            assert len(got[b]) == 0
            continue
        want = oracle.robust_prune(X, int(u), np.asarray(lst, dtype=np.uint32), m, alpha)
        assert got[b].tolist() == want.tolist(), (b, int(u), len(lst), m, alpha, presorted)
    return got


def clustered(dim, n=300, seed=0):
    rng = np.random.default_rng([seed, dim])
    X = (rng.standard_normal((10, dim))[np.arange(n) % 10] + 0.3 * rng.standard_normal((n, dim))).astype(np.float32)
    return rng, X


@BOTH
@DIMS
def test_short_lists_and_m_plus_one(ctx, oracle, dim, presorted):
    """Lists of 0, 1 and m are kept as they are; m + 1 is the first pruned
    length; 65 the sort's first size above one wave.  One launch."""
    m = 16
    rng, X = clustered(dim)
    lens = [0, 1, m, m + 1, 65]
    verts = np.array([299, 7, 150, 0, 19], dtype=np.uint32)
    lists = [rng.permutation(300)[:n].astype(np.uint32) for n in lens]
    got = check(ctx, oracle, X, verts, lists, m, 1.2, presorted)
    for g, lst in zip(got[:3], lists[:3]):
        assert g.tolist() == lst.tolist()


@BOTH
@DIMS
def test_two_accept_rounds_at_m64(ctx, oracle, dim, presorted):
    """m = 64 on lists of 200 far-apart rows: more than 32 are accepted, so the
    alpha test walks the accepted rows in two rounds of 32 groups.  Independent
    N(0,1) rows lie at 2 dim (1 +- sqrt(2 / dim)) from each other: at alpha 1.5 a
    rejection needs a 3.8 sigma pair at dim 257, so nearly all are accepted."""
    alpha = 1.5
    rng = np.random.default_rng(dim)
    X = rng.standard_normal((300, dim)).astype(np.float32)
    verts = rng.permutation(300)[:4].astype(np.uint32)
    lists = [rng.permutation(300)[:200].astype(np.uint32) for _ in verts]
    got = check(ctx, oracle, X, verts, lists, 64, alpha, presorted)
    for u, lst, g in zip(verts, lists, got):
        acc, _, _ = W.prune_trace(oracle, X, int(u), lst, 64, alpha)
        assert len(acc) > 32 and g[:len(acc)].tolist() == acc


@BOTH
@pytest.mark.parametrize("alpha", [1.0, 1.2, 2.0])
def test_rejected_by_an_accept_beyond_32(ctx, oracle, presorted, alpha):
    """late_rejector(dim=320): a candidate that only the 36th accepted neighbour
    rejects (m = 42): the alpha test must reach every accepted one."""
    X, cand, w, _ = W.late_rejector(dim=320)
    got = check(ctx, oracle, X, np.array([0], np.uint32), [cand], 42, alpha, presorted)
    assert got[0].tolist() == list(range(1, 43)) and w not in got[0].tolist()


@BOTH
@DIMS
def test_collinear_fill_from_discards(ctx, oracle, dim, presorted):
    """One accept, the other m - 1 from the discards in order."""
    m = 32
    X = W.collinear_points(100, dim)
    cand = np.random.default_rng(m).permutation(np.arange(1, 101)).astype(np.uint32)
    got = check(ctx, oracle, X, np.array([0], np.uint32), [cand], m, 1.2, presorted)
    assert got[0].tolist() == list(range(1, m + 1))


def test_presorted_discard_cap(ctx, oracle):
    """hub_discards(dim=257): more than 4,096 discards before the m-th accept
    (presorted): the kernel keeps 4,096 of them and needs none."""
    X, cand = W.hub_discards(dim=257)
    got = check(ctx, oracle, X, np.array([0], np.uint32), [cand], 8, 1.2, True)
    assert got[0].tolist() == [1] + list(range(4101, 4108))


def test_long_unsorted_list_sets_err(ctx, oracle):
    """A list above 4,096 by the kernel's own sort sets err and gets length 0;
    4,096 itself is sorted in LDS."""
    X, cand = W.hub_discards(dim=257)
    verts = np.array([0, 1], np.uint32)
    check(ctx, oracle, X, verts, [cand[:4097], cand[:4096]], 8, 1.2, False, expect_err=(0,))


@BOTH
def test_narrow_routing(ctx, presorted):
    """dim 64: pm_robust_prune_wide is pm_robust_prune."""
    import pacmann_amd as pm
    rng, X = clustered(64)
    verts = rng.permutation(300)[:6].astype(np.uint32)
    lists = [rng.permutation(300)[:100].astype(np.uint32) for _ in verts]
    a, ea = pm.robust_prune_wide(X, verts, lists, 32, 1.2, presorted, ctx)
    b, eb = pm.robust_prune(X, verts, lists, 32, 1.2, presorted, ctx)
    assert ea == eb == 0 and [x.tolist() for x in a] == [x.tolist() for x in b]
