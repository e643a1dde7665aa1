"""pm_knn_wide end to end against the oracle: rows of 193 to 1,024 dimensions
through the K-chunked prefilter k_knn_bf16x3_w, the certificate and the wide
brute-force kernel k_knn_brute<64, 1024>, on the tile, pad and chunk
edges; and the narrow routing for dim <= 192."""
import numpy as np
import pytest

from tests import knn_wide_ref as W

pytestmark = pytest.mark.gpu


def assert_equals_oracle(got_ids, got_d, want_ids, want_d):
    assert np.array_equal(got_ids, want_ids)
    assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32))


@pytest.mark.parametrize("n,nq,dim,k,integer", W.shape_cases())
def test_shape_edges(ctx, oracle, n, nq, dim, k, integer):
    """n and nq on the tile edges, dim on the pad and chunk edges, k = 1, 64 and
    one more (above n where n < 64); floats and integers 0..255 (from dim 259 on
    the integer sums pass 2^24); a duplicate row.  The oracle's ids and distance
    bits; beyond n the ids are -1 and the distances +inf; the wide prefilter ran."""
    import pacmann_amd as pm
    v, q = W.shape_data(n, nq, dim, integer)
    ctx.timing(1)
    try:
        ctx.timing_reset()
        gi, gd, fb = pm.knn_wide(v, q, k, ctx, with_dist=True)
        launches = ctx.timing_get("knn_prefilter_w")[0]
        narrow = ctx.timing_get("knn_prefilter_x3")[0]
    finally:
        ctx.timing(0)
    oi, od = oracle.knn(v, q, k)
    assert_equals_oracle(gi, gd, oi, od)
    assert launches >= 1 and narrow == 0
    if k > n:
        assert (gi[:, n:] == -1).all() and np.isposinf(gd[:, n:]).all() and (gi[:, :n] >= 0).all()
    if n <= 64:
        assert fb == 0
    assert 0 <= fb <= nq


@pytest.mark.parametrize("mirror", [False, True])
def test_descending_order_fills_the_insertion_buffer(ctx, oracle, mirror):
    """1,024 rows of dim 256 in descending distance order: every column of every
    tile goes into the row's insertion buffer (64 per tile, its width).  The
    mirror ascends: only the first tile inserts."""
    import pacmann_amd as pm
    v, q = W.descending_rows(256)
    if mirror:
        v = np.ascontiguousarray(v[::-1])
    q = np.repeat(q, 3, axis=0)
    for k in (1, 64):
        gi, gd, _ = pm.knn_wide(v, q, k, ctx, with_dist=True)
        oi, od = oracle.knn(v, q, k)
        assert_equals_oracle(gi, gd, oi, od)
    want = np.arange(64) if mirror else np.arange(1023, 959, -1)
    assert (gi == want).all()


def test_identical_rows_tie_by_id(ctx, oracle):
    """200 identical rows at dim 200 -> dp 256 and queries equal to them: the
    smallest ids win and exactly those queries are uncertified (more than 64
    rows share the 64th key's distance)."""
    import pacmann_amd as pm
    v, q, ntie = W.identical_rows()
    gi, gd, fb = pm.knn_wide(v, q, 1, ctx, with_dist=True)
    assert_equals_oracle(gi, gd, *oracle.knn(v, q, 1))
    assert fb == ntie
    gi, gd, fb = pm.knn_wide(v, q, 64, ctx, with_dist=True)
    assert_equals_oracle(gi, gd, *oracle.knn(v, q, 64))
    assert (gi[:ntie] == np.arange(10, 74)).all() and (gd[:ntie] == 0).all()
    assert fb >= ntie


@pytest.mark.parametrize("dim", [320, 1023])
def test_one_huge_row_uncertifies_all(ctx, oracle, dim):
    """One base row of norm about 2^100 among unit rows: eps follows the largest
    norm, so every row goes to k_knn_brute<64, 1024> (dim 320 = 5 x 64, dim 1,023 with a
    scalar tail of 7); the result is the oracle's."""
    import pacmann_amd as pm
    v, q = W.huge_row_data(dim)
    assert 2.0 ** 98 < W.norms64(v).max() < 2.0 ** 102
    ctx.timing(1)
    try:
        ctx.timing_reset()
        gi, gd, fb = pm.knn_wide(v, q, 10, ctx, with_dist=True)
        brute = ctx.timing_get("knn_brute")[0]
    finally:
        ctx.timing(0)
    assert_equals_oracle(gi, gd, *oracle.knn(v, q, 10))
    assert fb == len(q) and brute >= 1


@pytest.mark.parametrize("dim", [128, 192])
def test_narrow_routing(ctx, dim):
    """dim <= 192: pm_knn_wide is pm_knn_exact (ids, dists, fallback_rows), by
    the narrow prefilter."""
    import pacmann_amd as pm
    v, q = W.clustered_floats(1000, dim, nq=50)
    ctx.timing(1)
    try:
        ctx.timing_reset()
        wi, wd, wfb = pm.knn_wide(v, q, 48, ctx, with_dist=True)
        wide, narrow = ctx.timing_get("knn_prefilter_w")[0], ctx.timing_get("knn_prefilter_x3")[0]
    finally:
        ctx.timing(0)
    ei, ed, efb = pm.knn_exact(v, q, 48, ctx, with_dist=True)
    assert_equals_oracle(wi, wd, ei, ed)
    assert wfb == efb
    assert wide == 0 and narrow == 1
