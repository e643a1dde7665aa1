"""pm_kmeans against tests/kmeans_ref.py: centroid bits, labels, sizes and moved
are the reference's, whose update restates the documented f64 summation order
(members ascending, 16 partials p, p + 16, ..., partials added 0 .. 15)."""
import numpy as np
import pytest

from tests import kmeans_ref as R

pytestmark = pytest.mark.gpu


def assert_equals_ref(got, want):
    gc, gl, gs, gm = got
    wc, wl, ws, wm = want
    assert np.array_equal(gl, wl)
    assert np.array_equal(gs, ws)
    assert np.array_equal(gm, wm)
    assert np.array_equal(gc.view(np.uint32), wc.view(np.uint32))


wide_range_rows = R.wide_range_rows


def test_integer_rows(ctx, oracle):
    import pacmann_amd as pm
    rng = np.random.default_rng(1)
    rows = (rng.integers(0, 8, size=(600, 1)) * 40 + rng.integers(0, 30, size=(600, 128))).astype(np.float32)
    want = R.kmeans(rows, 17, 6, seed=3)
    assert_equals_ref(pm.kmeans(rows, 17, 6, seed=3, ctx=ctx), want)
    assert want[3][1] > 0   # the loop did move rows


@pytest.mark.parametrize("dim", [1, 7, 8, 200])
@pytest.mark.parametrize("nc", [1, 2, 129, 500])
def test_wide_range_rows(ctx, oracle, dim, nc):
    """nc = 129 exceeds the 128-key list (the certificate judges rows), nc = n makes every row a centroid;
    dim 1 and 7 have no 8-lane body, 200 is a wide row and two coordinate slices of the update."""
    import pacmann_amd as pm
    rows = wide_range_rows(500, dim, 10 * dim + nc)
    want = R.kmeans(rows, nc, 3, seed=5)
    assert_equals_ref(pm.kmeans(rows, nc, 3, seed=5, ctx=ctx), want)


def test_identical_init_centroids(ctx, oracle):
    """The higher of two identical centroids ends empty and keeps its value; ties go to the lower."""
    import pacmann_amd as pm
    rows, init = R.tied_init_case()
    got = pm.kmeans(rows, 3, 5, init=init, ctx=ctx)
    assert_equals_ref(got, R.kmeans(rows, 3, 5, init=init))
    assert got[2][1] == 0 and np.array_equal(got[0][1], init[1])


def test_niter_zero_labels_by_the_given_centroids(ctx, oracle):
    import pacmann_amd as pm
    rows = wide_range_rows(300, 24, 2)
    init = wide_range_rows(9, 24, 3)
    cen, labels, sizes, moved = pm.kmeans(rows, 9, 0, init=init, ctx=ctx)
    assert np.array_equal(cen.view(np.uint32), init.view(np.uint32))
    assert np.array_equal(labels, R.assign(rows, init))
    assert moved.tolist() == [300] and int(sizes.sum()) == 300


def test_early_stop_leaves_trailing_zeros(ctx, oracle):
    import pacmann_amd as pm
    rng = np.random.default_rng(6)
    gen = rng.integers(0, 4, size=400)
    rows = (gen[:, None] * 1000 + rng.integers(-20, 21, size=(400, 12))).astype(np.float32)
    got = pm.kmeans(rows, 4, 20, seed=9, ctx=ctx)
    assert_equals_ref(got, R.kmeans(rows, 4, 20, seed=9))
    moved = got[3]
    stop = int(np.flatnonzero(moved == 0)[0])
    assert 1 <= stop < 20 and (moved[stop:] == 0).all() and moved[0] == 400


def test_partial_sum_edges(ctx, oracle):
    """Clusters of exactly 15, 16, 17 and 33 members: one short partial, all
    partials once, one partial twice, and every partial twice plus one."""
    import pacmann_amd as pm
    sizes = [15, 16, 17, 33]
    gen = np.repeat(np.arange(4), sizes)
    np.random.default_rng(8).shuffle(gen)
    rows = np.zeros((len(gen), 10), np.float32)
    for c, size in enumerate(sizes):   # the cancelling pairs of wide_range_rows within each cluster
        rows[gen == c] = wide_range_rows(size, 10, 12 + c)
    rows[:, 0] = (gen * 2.0 ** 24).astype(np.float32)   # far apart: the clusters are the generating ones
    init = np.zeros((4, 10), np.float32)
    init[:, 0] = np.arange(4) * 2.0 ** 24
    got = pm.kmeans(rows, 4, 2, init=init, ctx=ctx)
    assert got[2].tolist() == sizes
    assert_equals_ref(got, R.kmeans(rows, 4, 2, init=init))


def test_two_calls_are_bit_identical(ctx):
    import pacmann_amd as pm
    rows = wide_range_rows(700, 33, 21)
    a = pm.kmeans(rows, 40, 5, seed=2, ctx=ctx)
    b = pm.kmeans(rows, 40, 5, seed=2, ctx=ctx)
    assert_equals_ref(a, b)
    assert a[3][1] > 0
