"""pm_knn_u8 end to end against the oracle on the rows as floats: k_u8_bias and
k_knn_i8 on the tile, pad and list edges of every row width,
on the extreme byte values, on ordered and tied rows, and against pm_knn_k128.
ids and distance bits are the oracle's everywhere: there is no fallback."""
import numpy as np
import pytest

from tests import knn_u8_ref as U

pytestmark = pytest.mark.gpu

F32 = np.float32


def assert_equals_oracle(got_ids, got_d, want_ids, want_d):
    assert np.array_equal(got_ids, want_ids)
    assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32))


def timed_knn(ctx, v, q, k):
    """(ids, dists, launches by timing name)."""
    import pacmann_amd as pm
    names = ("u8_bias", "knn_prefilter_u8", "u8_to_f32", "to_bf16", "knn_rerank", "knn_brute")
    ctx.timing(1)
    try:
        ctx.timing_reset()
        gi, gd = pm.knn_u8(v, q, k, ctx, with_dist=True)
        runs = {name: ctx.timing_get(name)[0] for name in names}
    finally:
        ctx.timing(0)
    return gi, gd, runs


@pytest.mark.parametrize("n,nq,dim,k", U.shape_cases())
def test_shape_edges(ctx, oracle, n, nq, dim, k):
    """n on the tile and list edges, nq on the block edges, dim on the edges of
    the four padded widths, k up to 128 and above n; a duplicate row.  Beyond n
    the ids are -1 and the distances +inf.  Two bias launches and the int8 kernel
    ran, and nothing of the float path."""
    v, q = U.shape_data(n, nq, dim)
    gi, gd, runs = timed_knn(ctx, v, q, k)
    oi, od = oracle.knn(v.astype(F32), q.astype(F32), k)
    assert_equals_oracle(gi, gd, oi, od)
    assert runs == {"u8_bias": 2, "knn_prefilter_u8": 1, "u8_to_f32": 0, "to_bf16": 0, "knn_rerank": 0, "knn_brute": 0}
    if k > n:
        assert (gi[:, n:] == -1).all() and np.isposinf(gd[:, n:]).all() and (gi[:, :n] >= 0).all()


def test_extreme_bytes_at_dim_256(ctx, oracle):
    """All 0, all 255 and 0/255 alternating: the largest accumulators of both
    signs, the largest constants and the distance 256 * 255^2."""
    import pacmann_amd as pm
    v, q = U.extreme_rows()
    for k in (1, 72, 128):
        gi, gd = pm.knn_u8(v, q, k, ctx, with_dist=True)
        assert_equals_oracle(gi, gd, *oracle.knn(v.astype(F32), q.astype(F32), k))
    assert gd[0, 71] == F32(U.MAX_DIST) and gd[0, 0] == 0 and np.isposinf(gd[:, 72:]).all()


@pytest.mark.parametrize("mirror", [False, True])
def test_descending_order_fills_the_insertion_buffer(ctx, oracle, mirror):
    """1,024 rows in strictly descending distance order: every column of every
    tile goes into the row's insertion buffer and moves all 128 keys.  The mirror
    ascends: only the first two tiles insert."""
    import pacmann_amd as pm
    v, q = U.descending_rows()
    if mirror:
        v = np.ascontiguousarray(v[::-1])
    q = np.repeat(q, 3, axis=0)
    for k in (1, 128):
        gi, gd = pm.knn_u8(v, q, k, ctx, with_dist=True)
        assert_equals_oracle(gi, gd, *oracle.knn(v.astype(F32), q.astype(F32), k))
    want = np.arange(128) if mirror else np.arange(1023, 895, -1)
    assert (gi == want).all()


def test_identical_rows_tie_by_id(ctx, oracle):
    """300 identical rows and queries equal to them: more than 128 rows share the
    128th key's distance and the smallest ids win."""
    import pacmann_amd as pm
    v, q, ntie = U.identical_rows()
    for k in (1, 128):
        gi, gd = pm.knn_u8(v, q, k, ctx, with_dist=True)
        assert_equals_oracle(gi, gd, *oracle.knn(v.astype(F32), q.astype(F32), k))
    assert (gi[:ntie] == np.arange(10, 138)).all() and (gd[:ntie] == 0).all()


def test_ties_at_one_distance_in_the_first_and_last_tile(ctx, oracle):
    """200 rows at distance 1, in the first tiles and in the last: the 128 kept
    are the 100 first and the 28 smallest ids of the last run."""
    import pacmann_amd as pm
    v, q, ids = U.one_distance_rows()
    for k in (100, 128):
        gi, gd = pm.knn_u8(v, q, k, ctx, with_dist=True)
        assert_equals_oracle(gi, gd, *oracle.knn(v.astype(F32), q.astype(F32), k))
    assert (gi[0] == ids[:128]).all() and (gd[0] == 1).all()


@pytest.mark.parametrize("dim", [100, 128])
def test_equals_the_float_path(ctx, dim):
    """n = 1,000: pm_knn_u8 equals pm_knn_k128 on the rows as floats."""
    import pacmann_amd as pm
    rng = np.random.default_rng([31, dim])
    v = rng.integers(0, 256, (1000, dim), dtype=np.uint8)
    q = rng.integers(0, 256, (70, dim), dtype=np.uint8)
    q[:5] = v[:5]
    for k in (10, 128):
        gi, gd = pm.knn_u8(v, q, k, ctx, with_dist=True)
        fi, fd, _ = pm.knn_k128(v.astype(F32), q.astype(F32), k, ctx, with_dist=True)
        assert_equals_oracle(gi, gd, fi, fd)


def test_rows_above_one_staging_piece(ctx, oracle):
    """140,000 rows of 256 bytes (35.8 MB) go up in two pieces of the 32 MiB
    staging buffer; ids across the piece boundary."""
    rng = np.random.default_rng(37)
    v = rng.integers(0, 256, (140_000, 256), dtype=np.uint8)
    q = np.stack([v[0], v[131_071], v[131_072], v[139_999], rng.integers(0, 256, 256, dtype=np.uint8)])
    gi, gd, runs = timed_knn(ctx, v, q, 10)
    assert_equals_oracle(gi, gd, *oracle.knn(v.astype(F32), q.astype(F32), 10))
    assert runs["u8_bias"] == 3 and runs["knn_prefilter_u8"] == 1
    assert list(gi[:4, 0]) == [0, 131_071, 131_072, 139_999]
