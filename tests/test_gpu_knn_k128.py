"""pm_knn_k128 end to end against the oracle: 128 prefilter keys per query row
(k_knn_bf16x3<DP, 128> for dp 128 / 192, k_knn_bf16x3_w<128, 32> above), the certificate
against the 128th prefilter distance and the 128-key brute-force kernels
(DESIGN.md §10.3), on the tile, pad, chunk and list edges, for k up to 128."""
import numpy as np
import pytest

from tests import knn_k128_ref as K

pytestmark = pytest.mark.gpu


def assert_equals_oracle(got_ids, got_d, want_ids, want_d):
    assert np.array_equal(got_ids, want_ids)
    assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32))


def timed_knn(ctx, v, q, k):
    """(ids, dists, fallback_rows, launches by timing name)."""
    import pacmann_amd as pm
    names = ("knn_prefilter_k128", "knn_prefilter_k128_w", "knn_prefilter_x3", "knn_prefilter_w", "knn_brute")
    ctx.timing(1)
    try:
        ctx.timing_reset()
        gi, gd, fb = pm.knn_k128(v, q, k, ctx, with_dist=True)
        runs = {name: ctx.timing_get(name)[0] for name in names}
    finally:
        ctx.timing(0)
    return gi, gd, fb, runs


@pytest.mark.parametrize("n,nq,dim,k,integer", K.shape_cases())
def test_shape_edges(ctx, oracle, n, nq, dim, k, integer):
    """n on the tile and list edges, nq on the block edges, dim on the pad and
    chunk edges of both prefilters, k up to 128 and above n; floats and integers
    0..255; a duplicate row.  The oracle's ids and distance bits; beyond n the
    ids are -1 and the distances +inf; no row is judged for n <= 128; the
    128-key prefilter of the row width ran and no 64-key one."""
    v, q = K.shape_data(n, nq, dim, integer)
    gi, gd, fb, runs = timed_knn(ctx, v, q, k)
    oi, od = oracle.knn(v, q, k)
    assert_equals_oracle(gi, gd, oi, od)
    mine, other = ("knn_prefilter_k128_w", "knn_prefilter_k128") if dim > 192 else \
        ("knn_prefilter_k128", "knn_prefilter_k128_w")
    assert runs[mine] == 1 and runs[other] == 0
    assert runs["knn_prefilter_x3"] == 0 and runs["knn_prefilter_w"] == 0
    if k > n:
        assert (gi[:, n:] == -1).all() and np.isposinf(gd[:, n:]).all() and (gi[:, :n] >= 0).all()
    if n <= K.TOP:
        assert fb == 0
    assert 0 <= fb <= nq


@pytest.mark.parametrize("dim", [100, 256])
@pytest.mark.parametrize("mirror", [False, True])
def test_descending_order_fills_the_insertion_buffer(ctx, oracle, mirror, dim):
    """1,024 rows in descending distance order: every column of every tile goes
    into the row's insertion buffer (64 per tile, its width) and moves all 128
    keys.  The mirror ascends: only the first two tiles insert."""
    import pacmann_amd as pm
    v, q = K.descending_rows(dim)
    if mirror:
        v = np.ascontiguousarray(v[::-1])
    q = np.repeat(q, 3, axis=0)
    for k in (1, 128):
        gi, gd, _ = pm.knn_k128(v, q, k, ctx, with_dist=True)
        oi, od = oracle.knn(v, q, k)
        assert_equals_oracle(gi, gd, oi, od)
    want = np.arange(128) if mirror else np.arange(1023, 895, -1)
    assert (gi == want).all()


@pytest.mark.parametrize("dim", [100, 200])
def test_identical_rows_tie_by_id(ctx, oracle, dim):
    """300 identical rows and queries equal to them: more than 128 rows share the
    128th key's distance, the smallest ids win and exactly those queries are
    uncertified at k = 1."""
    import pacmann_amd as pm
    v, q, ntie = K.identical_rows(dim)
    gi, gd, fb = pm.knn_k128(v, q, 1, ctx, with_dist=True)
    assert_equals_oracle(gi, gd, *oracle.knn(v, q, 1))
    assert fb == ntie
    gi, gd, fb = pm.knn_k128(v, q, 128, ctx, with_dist=True)
    assert_equals_oracle(gi, gd, *oracle.knn(v, q, 128))
    assert (gi[:ntie] == np.arange(10, 138)).all() and (gd[:ntie] == 0).all()
    assert fb >= ntie


@pytest.mark.parametrize("dim", [100, 320, 1023])
def test_one_huge_row_uncertifies_all(ctx, oracle, dim):
    """One base row of norm about 2^100 among unit rows: eps follows the largest
    norm, so every row goes to the 128-key brute-force kernel (dim 100: the
    192-float query row and a scalar tail of 4; 320: the 1,024-float one, no
    tail; 1,023: a tail of 7); k = 100 reads both halves of the merged list."""
    v, q = K.huge_row_data(dim)
    assert 2.0 ** 98 < K.norms64(v).max() < 2.0 ** 102
    gi, gd, fb, runs = timed_knn(ctx, v, q, 100)
    assert_equals_oracle(gi, gd, *oracle.knn(v, q, 100))
    assert fb == len(q) and runs["knn_brute"] >= 1
