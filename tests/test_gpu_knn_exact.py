"""pm_knn_exact and pm_build_graph_exact: the brute-force (L2Dist, id) ranking
for general float rows, through the certified prefilter or the brute-force
fallback, and the shape, order, tie and scale edges of both
kNN paths end to end.  NaN and infinite inputs are out of contract: they get
some answer through the fallback, and no test here feeds them."""
import ctypes as C

import numpy as np
import pytest

from tests import knn_ref as R
from tests.knn_ref import clustered_floats, near_duplicate_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clustered(oracle):
    v, q = clustered_floats(4000, 192, nq=50)
    assert q.shape == (50, 192)
    oi, od = oracle.knn(v, q, 64)
    return v, q, oi, od


def assert_equals_oracle(got_ids, got_d, want_ids, want_d):
    assert np.array_equal(got_ids, want_ids)
    assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32))


def test_clustered_floats_fast_path(ctx, clustered):
    """Clustered float rows, k = 10: ids and distance bits of brute force, and
    no more fallback rows than queries whose margin d64 - d10 is below twice
    the contract bound 2^-12 (|q|^2 + max |x|^2) (none on this data)."""
    import pacmann_amd as pm
    v, q, oi, od = clustered
    gi, gd, fb = pm.knn_exact(v, q, 10, ctx, with_dist=True)
    assert_equals_oracle(gi, gd, oi[:, :10], od[:, :10])
    margin = od[:, 63].astype(np.float64) - od[:, 9]
    v64, q64 = v.astype(np.float64), q.astype(np.float64)
    bound = 2.0 ** -12 * ((q64 * q64).sum(1) + (v64 * v64).sum(1).max())
    cap = int((margin < 2 * bound).sum())
    print(f"margin min {margin.min():.3f} median {np.median(margin):.3f}, bound median {np.median(bound):.3f}, "
          f"cap {cap}, fallback_rows {fb}")
    assert cap == 0
    assert fb <= cap


def test_clustered_floats_k48(ctx, clustered):
    """The same rows at the graph build's K = 48: margins (0.04-0.08) are below
    the contract bound, so rows reach the fallback; results equal brute force."""
    import pacmann_amd as pm
    v, q, oi, od = clustered
    gi, gd, fb = pm.knn_exact(v, q, 48, ctx, with_dist=True)
    print(f"k=48 fallback_rows {fb} of {len(q)}")
    assert_equals_oracle(gi, gd, oi[:, :48], od[:, :48])
    assert 0 <= fb <= len(q)


def test_forced_fallback_ragged_dim(ctx, oracle):
    """100 rows within a few ulps of one row (more than 64 within any eps of
    the first four queries): no certificate can hold, the brute-force kernel
    answers them, id-order ties included; dim % 8 != 0."""
    import pacmann_amd as pm
    v, q = near_duplicate_rows()
    gi, gd, fb = pm.knn_exact(v, q, 20, ctx, with_dist=True)
    oi, od = oracle.knn(v, q, 20)
    assert_equals_oracle(gi, gd, oi, od)
    assert fb >= 4, fb


@pytest.mark.parametrize("n,d,k", [(40, 16, 20), (65, 8, 64), (777, 100, 1)])
def test_small_and_edge_shapes(ctx, oracle, n, d, k):
    """n < 64 (everything kept, no fallback), n = 65 with k = 64, a ragged dim
    with k = 1; duplicate rows (ties -> id order)."""
    import pacmann_amd as pm
    rng = np.random.default_rng(n)
    v = rng.standard_normal((n, d)).astype(np.float32)
    v[5] = v[3]
    q = np.concatenate([v[:8], rng.standard_normal((9, d)).astype(np.float32)])
    gi, gd, fb = pm.knn_exact(v, q, k, ctx, with_dist=True)
    oi, od = oracle.knn(v, q, k)
    assert_equals_oracle(gi, gd, oi, od)
    if n <= 64:
        assert fb == 0


def test_integer_rows_equal_knn(ctx):
    """Integer-valued rows (exact in bf16): the same ids and distance bits as pm_knn."""
    import pacmann_amd as pm
    from tests.datagen import clustered_vectors
    v = clustered_vectors(1500, 192, seed=1500)
    q = np.clip(v[::25][:60] + 1, 0, 255).astype(np.float32)
    gi, gd, _ = pm.knn_exact(v, q, 20, ctx, with_dist=True)
    ki, kd = pm.knn(v, q, 20, ctx, with_dist=True)
    assert_equals_oracle(gi, gd, ki, kd)
    ids_only, fb = pm.knn_exact(v, q, 20, ctx)
    assert np.array_equal(ids_only, ki) and isinstance(fb, int)


@pytest.mark.parametrize("n,d,m,centres", [(1200, 192, 32, 20), (500, 100, 16, 10)])
def test_build_graph_exact_on_floats(ctx, oracle, n, d, m, centres):
    """pm_build_graph_exact on clustered float rows: the oracle's graph row for
    row, no row lists itself, the fallback count is reported."""
    import pacmann_amd as pm
    v = clustered_floats(n, d, centres=centres)
    g, t = pm.build_graph(v, m, 1.2, seed=9, ctx=ctx, exact=True)
    o = oracle.build_graph(v, m, 1.2, seed=9)
    print(f"n={n} d={d} m={m}: knn_fallback_rows {t['knn_fallback_rows']}")
    if not np.array_equal(g, o):
        bad = np.where((g != o).any(axis=1))[0]
        pytest.fail(f"{len(bad)} rows differ, first {bad[:5].tolist()}: {g[bad[0]].tolist()} vs {o[bad[0]].tolist()}")
    assert (g != np.arange(n, dtype=np.uint32)[:, None]).all()
    assert 0 <= t["knn_fallback_rows"] <= n
    assert t["knn_s"] > 0


@pytest.mark.parametrize("n,nq,dim,k,kc", R.shape_cases())
def test_shape_edges(ctx, oracle, n, nq, dim, k, kc):
    """n and nq on the tile edges, dim on the chunk and pad edges, k = 1, 64 and
    one more (above n where n < 63): the oracle's ids and distance bits; beyond
    n the ids are -1 and the distances +inf."""
    import pacmann_amd as pm
    v, q = R.shape_data(n, nq, dim, integer=False)
    gi, gd, fb = pm.knn_exact(v, q, k, ctx, with_dist=True)
    oi, od = oracle.knn(v, q, k)
    assert_equals_oracle(gi, gd, oi, od)
    if k > n:
        assert (gi[:, n:] == -1).all() and np.isposinf(gd[:, n:]).all() and (gi[:, :n] >= 0).all()
    if n <= 64:
        assert fb == 0


@pytest.mark.parametrize("mirror", [False, True])
def test_descending_order_fills_the_insertion_buffer(ctx, oracle, mirror):
    """Base rows in descending distance order: every column of every tile goes
    into the row's insertion buffer (64 per tile, its width).  The mirror
    ascends: only the first tile inserts."""
    import pacmann_amd as pm
    v, q = R.descending_rows(integer=False)
    if mirror:
        v = np.ascontiguousarray(v[::-1])
    q = np.repeat(q, 3, axis=0)
    for k in (1, 64):
        gi, gd, _ = pm.knn_exact(v, q, k, ctx, with_dist=True)
        oi, od = oracle.knn(v, q, k)
        assert_equals_oracle(gi, gd, oi, od)
    want = np.arange(64) if mirror else np.arange(1023, 959, -1)
    assert (gi == want).all()


def test_identical_rows_tie_by_id(ctx, oracle):
    """200 identical rows and queries equal to them: the smallest ids win, and
    exactly those queries are uncertified (more than 64 rows share the 64th
    key's distance); a query equal to a lone base row is certified at k = 1."""
    import pacmann_amd as pm
    v, q, ntie = R.identical_rows(integer=False)
    gi, gd, fb = pm.knn_exact(v, q, 1, ctx, with_dist=True)
    assert_equals_oracle(gi, gd, *oracle.knn(v, q, 1))
    assert fb == ntie
    gi, gd, fb = pm.knn_exact(v, q, 64, ctx, with_dist=True)
    assert_equals_oracle(gi, gd, *oracle.knn(v, q, 64))
    assert (gi[:ntie] == np.arange(10, 74)).all() and (gd[:ntie] == 0).all()
    assert fb >= ntie


def test_equidistant_rows_tie_by_id(ctx, oracle):
    """200 rows at one exact non-zero L2Dist, in the first and the last tiles:
    the prefilter's own distances of them differ, the certificate must refuse
    the rows, and the smallest ids win."""
    import pacmann_amd as pm
    v, q, ntie = R.equidistant_rows(integer=False)
    for k in (1, 64):
        gi, gd, fb = pm.knn_exact(v, q, k, ctx, with_dist=True)
        assert_equals_oracle(gi, gd, *oracle.knn(v, q, k))
        assert fb == ntie == len(q)
    assert (gi == np.arange(64)).all() and (gd == np.float32(0.25)).all()


@pytest.mark.parametrize("exp", [-70, -25, 30, 58])
def test_scaled_rows(ctx, oracle, exp):
    """The clustered rows times a power of two: ids and distance bits of the
    oracle (2^-70: the distances are f32 subnormals and the 2^-50 term is the
    whole eps, so every row is uncertified; 2^58: the sums stay below 2^126)."""
    import pacmann_amd as pm
    v, q = clustered_floats(1000, 100, nq=50)
    s = np.float32(2.0) ** np.float32(exp)
    v, q = v * s, q * s
    oi, od = oracle.knn(v, q, 10)
    assert np.isfinite(od).all()
    if exp == -70:
        assert (od < 2.0 ** -126).all() and (od > 0).all()
    gi, gd, fb = pm.knn_exact(v, q, 10, ctx, with_dist=True)
    print(f"scale 2^{exp}: fallback_rows {fb} of {len(q)}")
    assert_equals_oracle(gi, gd, oi, od)
    if exp == -70:
        assert fb == len(q)


def test_one_huge_row_uncertifies_all(ctx, oracle):
    """One base row of norm about 2^100 among unit rows: eps follows the largest
    norm, far above every distance, so every row goes to the fallback."""
    import pacmann_amd as pm
    v, q = clustered_floats(1000, 100, nq=50)
    v[500] = v[500] * np.float32(2.0 ** 47)   # |x|^2 about 100 * 2^94
    assert 2.0 ** 99 < R.norms64(v[500:501])[0] < 2.0 ** 102
    gi, gd, fb = pm.knn_exact(v, q, 10, ctx, with_dist=True)
    assert_equals_oracle(gi, gd, *oracle.knn(v, q, 10))
    assert fb == len(q)


def test_overflowing_norms_uncertify_all(ctx, oracle):
    """Scale 2^62: the norms overflow, sum <= 2^126 fails for every row; the
    oracle's +inf distances are ranked by id."""
    import pacmann_amd as pm
    v, q = clustered_floats(1000, 100, nq=50)
    s = np.float32(2.0 ** 62)
    v, q = v * s, q * s
    assert np.isfinite(v).all() and np.isfinite(q).all() and R.norms64(v).min() > R.MAX_SUM
    oi, od = oracle.knn(v, q, 64)   # 50 rows per cluster at finite distances, then +inf by id
    assert np.isposinf(od[:, 50:]).all() and np.isfinite(od[:, :40]).all()
    gi, gd, fb = pm.knn_exact(v, q, 64, ctx, with_dist=True)
    assert_equals_oracle(gi, gd, oi, od)
    assert fb == len(q)


def test_argument_checks(ctx):
    """PM_EINVAL with a text, before any HIP call."""
    import pacmann_amd as pm
    L = pm.lib()
    PM_EINVAL = -1
    v = np.zeros((64, 193), dtype=np.float32)
    ids = np.zeros((1, 65), dtype=np.int64)
    g = np.zeros((64, 43), dtype=np.uint32)
    fb = C.c_uint64(7)
    f32p, i64p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_uint32)
    vp, ip, gp = v.ctypes.data_as(f32p), ids.ctypes.data_as(i64p), g.ctypes.data_as(u32p)
    cases = [
        (lambda: L.pm_knn_exact(None, vp, 64, 16, vp, 1, 10, ip, None, C.byref(fb)), b"NULL argument"),
        (lambda: L.pm_knn_exact(ctx.h, vp, 64, 16, vp, 1, 0, ip, None, C.byref(fb)), b"k must be in [1, 64]"),
        (lambda: L.pm_knn_exact(ctx.h, vp, 64, 16, vp, 1, 65, ip, None, C.byref(fb)), b"k must be in [1, 64]"),
        (lambda: L.pm_knn_exact(ctx.h, vp, 64, 193, vp, 1, 10, ip, None, C.byref(fb)), b"kNN supports dim <= 192"),
        (lambda: L.pm_build_graph_exact(None, vp, 64, 16, 8, 1.2, 1, gp, None, C.byref(fb)), b"NULL argument"),
        (lambda: L.pm_build_graph_exact(ctx.h, vp, 64, 16, 43, 1.2, 1, gp, None, C.byref(fb)), b"m must be in [1, 42]"),
        (lambda: L.pm_build_graph_exact(ctx.h, vp, 64, 193, 8, 1.2, 1, gp, None, C.byref(fb)),
         b"dim must be in [1, 192]"),
    ]
    for call, want in cases:
        assert L.pm_ctx_mem_info(None, None, None) == PM_EINVAL   # another text first
        assert call() == PM_EINVAL
        assert L.pm_last_error().startswith(want), L.pm_last_error()
