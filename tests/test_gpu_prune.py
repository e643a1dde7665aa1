"""k_prune against oracle.robust_prune vertex by vertex, through
pm_robust_prune: by the kernel's own LDS sort and in the presorted form the
build uses for hub lists (k_cand_dist, host sort, the same greedy pass)."""
import ctypes as C

import numpy as np
import pytest

from tests import knn_ref as R

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("presorted", [False, True], ids=["lds_sort", "presorted"])


def check(ctx, oracle, X, verts, lists, m, alpha, presorted, expect_err=()):
    """Every list's result equals the oracle's; the lists in expect_err (above
    the LDS sort's limit, unsorted form) give length 0 and raise the flag."""
    import pacmann_amd as pm
    got, err = pm.robust_prune(X, verts, lists, m, alpha, presorted, ctx)
    assert err == (1 if len(expect_err) else 0)
    for b, (u, lst) in enumerate(zip(verts, lists)):
        if b in expect_err:
            assert len(got[b]) == 0
            continue
        want = oracle.robust_prune(X, int(u), np.asarray(lst, dtype=np.uint32), m, alpha)
        assert got[b].tolist() == want.tolist(), (b, int(u), len(lst), m, alpha, presorted)
    return got


@BOTH
def test_list_lengths(ctx, oracle, presorted):
    """Lengths 0, 1, m and m + 1 (the copy path and the first pruned length), 63,
    64 and 65 (the sort's smallest padded size), 4,096 (the limit) and 4,097:
    the error flag unsorted, the oracle's list presorted.  One launch, the
    vertices out of order."""
    m = 32
    rng = np.random.default_rng(8)
    X = rng.standard_normal((4200, 8)).astype(np.float32)
    lens = [0, 1, m, m + 1, 63, 64, 65, 4096, 4097]
    verts = np.array([4100, 7, 3000, 0, 19, 4199, 64, 2, 1], dtype=np.uint32)
    lists = [rng.permutation(4200)[:n].astype(np.uint32) for n in lens]
    check(ctx, oracle, X, verts, lists, m, 1.2, presorted, expect_err=() if presorted else (8,))


@BOTH
@pytest.mark.parametrize("dim", [1, 7, 8, 100, 192, 256])
def test_m_alpha_dim(ctx, oracle, dim, presorted):
    """m in {1, 32, 42, 64} x alpha in {1.0, 1.2, 2.0} at each dim (the 8-lane
    L2Dist's tail, the widest row); lists of 100 from 300 clustered rows, so
    that the alpha test both accepts and rejects."""
    rng = np.random.default_rng(dim)
    X = (rng.standard_normal((10, dim))[np.arange(300) % 10] + 0.3 * rng.standard_normal((300, dim))).astype(np.float32)
    verts = rng.permutation(300)[:12].astype(np.uint32)
    lists = [rng.permutation(300)[:100].astype(np.uint32) for _ in verts]
    for m in (1, 32, 42, 64):
        for alpha in (1.0, 1.2, 2.0):
            got = check(ctx, oracle, X, verts, lists, m, alpha, presorted)
            assert all(len(g) == m for g in got)   # accepted ones, then discards up to m


@BOTH
def test_repeats_equal_distances_and_self(ctx, oracle, presorted):
    """Lists with repeated ids, distinct ids at equal distance (equal rows) and
    the vertex itself (distance 0: accepted): positional order decides."""
    rng = np.random.default_rng(12)
    X = rng.standard_normal((200, 7)).astype(np.float32)
    X[50:60] = X[40:50]            # ten pairs of distinct ids with equal rows
    X[150:160] = X[3]              # ten copies of vertex 3's own row
    verts = np.array([3, 120, 45, 0], dtype=np.uint32)
    lists = []
    for u in verts:
        lst = np.concatenate([rng.integers(0, 200, 60), np.arange(40, 60), np.arange(150, 160), [u, u],
                              rng.integers(0, 200, 30)]).astype(np.uint32)
        lists.append(rng.permutation(np.concatenate([lst, lst[:25]])))
    for m, alpha in ((8, 1.2), (32, 1.0), (64, 2.0)):
        got = check(ctx, oracle, X, verts, lists, m, alpha, presorted)
        # vertex 3's list holds itself and ten copies of its row at least 12 times: 0 * alpha < 0 is false, so
        # the distance-0 run is accepted whole, in list order
        assert (X[got[0][:min(m, 12)]] == X[3]).all()


@BOTH
@pytest.mark.parametrize("m,alpha", [(8, 1.0), (32, 1.2), (64, 2.0)])
def test_collinear_fill_from_discards(ctx, oracle, presorted, m, alpha):
    """One accept, the other m - 1 from the discards in order."""
    X = R.collinear_points(100)
    rng = np.random.default_rng(m)
    cand = rng.permutation(np.arange(1, 101)).astype(np.uint32)
    got = check(ctx, oracle, X, np.array([0], np.uint32), [cand], m, alpha, presorted)
    assert got[0].tolist() == list(range(1, m + 1))


@BOTH
@pytest.mark.parametrize("alpha", [1.0, 1.2, 2.0])
def test_rejected_by_an_accept_beyond_32(ctx, oracle, presorted, alpha):
    """A candidate that only the 36th accepted neighbour rejects (m = 42, the
    build's largest): the alpha test must reach every accepted one, not only a
    first round of 32 (256 threads / 8 lanes)."""
    X, cand, w, _ = R.late_rejector()
    got = check(ctx, oracle, X, np.array([0], np.uint32), [cand], 42, alpha, presorted)
    assert got[0].tolist() == list(range(1, 43)) and w not in got[0].tolist()


def test_presorted_discard_cap(ctx, oracle):
    """More than 4,096 discards before the m-th accept (presorted): the kernel
    keeps 4,096 of them and needs none; and the same line alone, where the
    first m - 1 discards fill the list."""
    X, cand = R.hub_discards()
    got = check(ctx, oracle, X, np.array([0], np.uint32), [cand], 8, 1.2, True)
    assert got[0].tolist() == [1] + list(range(4101, 4108))
    got = check(ctx, oracle, X, np.array([0], np.uint32), [cand[:4100]], 8, 1.2, True)
    assert got[0].tolist() == list(range(1, 9))


def test_argument_checks(ctx):
    """PM_EINVAL with a text, before any HIP call."""
    import pacmann_amd as pm
    L = pm.lib()
    X = np.zeros((10, 8), np.float32)
    verts, dup, far = (np.array(a, np.uint32) for a in ([1, 2], [1, 1], [1, 10]))
    offs, lens = np.array([0, 2], np.uint64), np.array([2, 2], np.uint32)
    ids, bad = np.array([3, 4, 5, 6], np.uint32), np.array([3, 4, 5, 10], np.uint32)
    out, ol, err = np.zeros((2, 64), np.uint32), np.zeros(2, np.uint32), np.zeros(1, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p).value   # noqa: E731
    cast = lambda a, t: C.cast(p(a), t)                 # noqa: E731
    f, u32, u64 = pm.f32p, pm.u32p, pm.u64p

    def call(ctxh=ctx.h, n=10, dim=8, v=verts, nv=2, o=offs, ln=lens, i=ids, ni=4, m=4):
        return L.pm_robust_prune(ctxh, cast(X, f), n, dim, cast(v, u32), nv, cast(o, u64), cast(ln, u32), cast(i, u32), ni,
                                 m, 1.2, 0, cast(out, u32), cast(ol, u32), cast(err, u32))
    cases = [
        (lambda: call(ctxh=None), b"NULL argument"),
        (lambda: call(m=0), b"m must be in [1, 64]"),
        (lambda: call(m=65), b"m must be in [1, 64]"),
        (lambda: call(dim=0), b"dim must be in [1, 256]"),
        (lambda: call(dim=257), b"dim must be in [1, 256]"),
        (lambda: call(n=0), b"n must be in [1, 2^32-1)"),
        (lambda: call(nv=0), b"nverts must be in [1, n]"),
        (lambda: call(i=bad), b"candidate id out of range"),
        (lambda: call(v=far), b"vertex out of range"),
        (lambda: call(v=dup), b"verts must be distinct"),
        (lambda: call(ni=3), b"list outside ids"),
    ]
    for fn, want in cases:
        assert L.pm_ctx_mem_info(None, None, None) == -1   # another text first
        assert fn() == -1
        assert L.pm_last_error().startswith(want), L.pm_last_error()
