"""pm_cluster_* against tests/kmeans_ref.py (cluster_search): the probed
clusters, ids, distance bits and scanned rows are the reference's, on clusters
built by hand through `labels` whose sizes sit on the edges of the scan's
eight-row groups (0, 1, 7, 8, 9, 31, 32, 33) and go up to several hundred."""
import numpy as np
import pytest

from tests import kmeans_ref as R

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 7, 8, 9, 31, 32, 33, 0, 300, 400, 679]   # 1,500 rows
NC = len(SIZES)
EMPTY, SINGLE, TWIN_A, TWIN_B = 8, 1, 9, 10


class Case:
    def __init__(self, dim):
        import pacmann_amd as pm
        rng = np.random.default_rng(100 + dim)
        self.labels = np.repeat(np.arange(NC), SIZES).astype(np.int64)
        rng.shuffle(self.labels)
        n = len(self.labels)
        centre = rng.uniform(-50, 50, size=(NC, dim))
        self.rows = (centre[self.labels] + rng.normal(0, 4, size=(n, dim))).astype(np.float32)
        # identical rows in two clusters, the higher id in the lower cluster
        a, b = np.flatnonzero(self.labels == TWIN_A)[-1], np.flatnonzero(self.labels == TWIN_B)[0]
        assert a != b
        self.twins = (min(a, b), max(a, b))
        self.rows[a] = self.rows[b]
        self.cen = centre.astype(np.float32)
        self.cen[EMPTY] = 900.0    # an empty cluster far from every row
        single = self.rows[self.labels == SINGLE][0]
        self.cen[SINGLE] = single
        self.queries = np.vstack([
            self.rows[3] + 0.5, centre[11].astype(np.float32), self.rows[self.twins[0]],
            self.cen[EMPTY] + 1, single + 0.25, rng.uniform(-60, 60, size=(3, dim))]).astype(np.float32)
        self.index = pm.ClusterIndex(self.rows, self.cen, self.labels)


@pytest.fixture(scope="module", params=[8, 128, 200])
def case(request, ctx, oracle):
    c = Case(request.param)
    yield c
    c.index.close()


@pytest.mark.parametrize("nprobe", [1, 3, NC])
@pytest.mark.parametrize("k", [1, 10, 128])
def test_equals_reference(case, k, nprobe):
    ids, d, pr, sc = case.index.search(case.queries, k, nprobe, with_dist=True, with_probed=True)
    wi, wd, wp, ws = R.cluster_search(case.rows, case.cen, case.labels, case.queries, k, nprobe)
    assert np.array_equal(pr, wp)
    assert np.array_equal(sc, ws)
    assert np.array_equal(ids, wi)
    assert np.array_equal(d.view(np.uint32), wd.view(np.uint32))


@pytest.mark.parametrize("k", [1, 10, 128])
def test_all_clusters_equal_exact_knn(case, ctx, k):
    import pacmann_amd as pm
    ids, d = case.index.search(case.queries, k, NC, with_dist=True)
    wi, wd, _ = pm.knn_k128(case.rows, case.queries, k, ctx, with_dist=True)
    assert np.array_equal(ids, wi)
    assert np.array_equal(d.view(np.uint32), wd.view(np.uint32))


def test_padding(case):
    """Query 3 sits on the empty cluster's centroid: nothing scanned, every id -1.  Query 4 sits on the
    one-row cluster: one answer, then padding."""
    ids, d, pr, sc = case.index.search(case.queries, 10, 1, with_dist=True, with_probed=True)
    assert pr[3, 0] == EMPTY and sc[3] == 0 and (ids[3] == -1).all() and np.isposinf(d[3]).all()
    assert pr[4, 0] == SINGLE and sc[4] == 1 and ids[4, 0] >= 0 and (ids[4, 1:] == -1).all()
    assert np.isfinite(d[4, 0]) and np.isposinf(d[4, 1:]).all()
    ids3, _, sc3 = case.index.search(case.queries[3:5], 128, 3, with_probed=True)
    assert ((ids3 >= 0).sum(axis=1) == np.minimum(128, sc3)).all() and (sc3 > 0).all()


def test_identical_rows_rank_by_original_id(case):
    ids, d = case.index.search(case.queries[2], 2, NC, with_dist=True)
    assert tuple(ids[0]) == case.twins and d[0, 0] == 0 and d[0, 1] == 0


def test_info_is_the_stable_order(case):
    assert np.array_equal(case.index.order, np.argsort(case.labels, kind="stable"))
    assert np.array_equal(case.index.offsets, np.concatenate([[0], np.cumsum(SIZES)]))


def test_argument_rules_that_need_an_index(case):
    for k, nprobe in ((10, 0), (10, NC + 1), (0, 1), (129, 1)):
        with pytest.raises(RuntimeError, match="must be in"):
            case.index.search(case.queries, k, nprobe)


def test_kernels_ran_once(case, ctx):
    import pacmann_amd as pm
    ctx.timing(1)
    try:
        ctx.timing_reset()
        idx = pm.ClusterIndex(case.rows, case.cen, case.labels, ctx)
        assert ctx.timing_get("cluster_gather")[0] == 1 and ctx.timing_get("cluster_scan")[0] == 0
        idx.search(case.queries, 10, 3)
        assert ctx.timing_get("cluster_gather")[0] == 1 and ctx.timing_get("cluster_scan")[0] == 1
        idx.close()
    finally:
        ctx.timing(0)


def test_save_load_round_trip(case, tmp_path):
    import pacmann_amd as pm
    prefix = str(tmp_path / "sift")
    case.index.save(prefix)
    np.save(prefix + "-labels.npy", case.labels.astype(np.int64))   # faiss writes int64
    other = pm.ClusterIndex.load(prefix, case.rows)
    a = case.index.search(case.queries, 10, 3, with_dist=True, with_probed=True)
    b = other.search(case.queries, 10, 3, with_dist=True, with_probed=True)
    other.close()
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                              y.view(np.uint32) if y.dtype == np.float32 else y)


def test_a_cluster_in_several_pieces(ctx, oracle):
    """A cluster above the scan's 2,048-row work item is scanned in pieces and merged."""
    import pacmann_amd as pm
    rng = np.random.default_rng(5)
    rows = rng.integers(-30, 31, size=(5000, 8)).astype(np.float32)   # many exact ties
    labels = np.where(np.arange(5000) % 10 == 0, 0, 1)
    cen = np.vstack([rows[labels == c].mean(0) for c in (0, 1)]).astype(np.float32)
    q = rows[[1, 7, 4999]] + np.float32(0.5)
    idx = pm.ClusterIndex(rows, cen, labels, ctx)
    for k, nprobe in ((128, 1), (10, 2)):
        ids, d, pr, sc = idx.search(q, k, nprobe, with_dist=True, with_probed=True)
        wi, wd, wp, ws = R.cluster_search(rows, cen, labels, q, k, nprobe)
        assert np.array_equal(pr, wp) and np.array_equal(sc, ws) and np.array_equal(ids, wi)
        assert np.array_equal(d.view(np.uint32), wd.view(np.uint32))
    idx.close()


def test_train_and_recall(ctx):
    """Not bit-exact: the trained index finds some but not all true neighbours from one cluster of 64,
    and all of them from all clusters."""
    import pacmann_amd as pm
    from pacmann_amd import report, synth
    v = synth.clustered_vectors(4096, 32)
    q = v[::64] + np.float32(0.5)
    idx = pm.ClusterIndex.train(v, ctx=ctx)
    assert idx.nc == 64 and int(idx.offsets[-1]) == 4096
    gnd = pm.knn(v, q, 10, ctx)
    r1 = report.compute_recall(gnd, idx.search(q, 10, 1), 10)
    rall = report.compute_recall(gnd, idx.search(q, 10, idx.nc), 10)
    idx.close()
    assert 0.0 < r1 < 1.0
    assert rall == 1.0
