"""GraphANNFrontend.SearchKNNBatch (graphann/search.go:236-245) on the device:
pm_search_knn_batch / PIRGraphInfo.SearchKNNBatch runs a whole non-private
SearchKNN per workgroup (k_knn_batch, pm_knnb.hip).  Its result is defined as
the loop of SearchKNN, so every test runs the batch call on the product and
the per-query loop on the oracle, built with the same seeds, and asserts equal
ids, reach steps and counters.

A search draws from the graph's id stream only where a pop finds its heap
empty; the kernel hands such queries back to the host.  Whether that happens
depends on the data alone, so the seeds below are chosen (and checked here on
the CPU side, through the oracle's start set after a second Preprocess) such
that the shapes meant for the kernel draw nothing: `device_queries == nq`
then shows that the kernel, not the host loop, gave the answers."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _pair(ctx, oracle, v, g, nonprivate=True, pir_seed=5, search_seed=6):
    import pacmann_amd as pm
    gi = pm.PIRGraphInfo(v, g, nonprivate=nonprivate, pir_seed=pir_seed, search_seed=search_seed, ctx=ctx)
    og = oracle.Graph(v, g, nonprivate=nonprivate, pir_seed=pir_seed, search_seed=search_seed)
    gi.Preprocess()
    og.Preprocess()
    return gi, og


def _same(gi, og, qs, k, steps, par, benchmarking=False):
    """The batch call against the oracle's loop; returns (ids, steps, device_queries)."""
    qs = np.ascontiguousarray(qs, dtype=np.float32)
    ids, st, dq = gi.SearchKNNBatch(qs, k, steps, par, benchmarking, return_device_queries=True)
    assert ids.shape == st.shape == (len(qs), k)
    for i, q in enumerate(qs):
        wi, ws = og.SearchKNN(q, k, steps, par, benchmarking)
        assert np.array_equal(ids[i], wi), (i, ids[i], wi)
        assert np.array_equal(st[i], ws), (i, st[i], ws)
    assert gi.counts() == og.counts()
    return ids, st, dq


def _oracle_drew_nothing(oracle, og, v, g, pir_seed=5, search_seed=6):
    """A second Preprocess redraws the start set from the id stream: the same
    start set as an unsearched twin's means that no search of `og` drew an id."""
    twin = oracle.Graph(v, g, nonprivate=True, skip_prep=True, pir_seed=pir_seed, search_seed=search_seed)
    twin.Preprocess()
    twin.Preprocess()
    og.Preprocess()
    return np.array_equal(og.GetStartVertex()[0], twin.GetStartVertex()[0])


@functools.lru_cache(maxsize=None)
def _base():
    from pacmann_amd.synth import knn_graph, sift_like_vectors
    v = sift_like_vectors(4096, 128, seed=11)
    g = knn_graph(v, 32)
    v.setflags(write=False)
    g.setflags(write=False)
    return v, g


def small_shape():
    """Shape 5: at most 64 vertices to push against 80 pops, so every query draws."""
    from pacmann_amd.synth import knn_graph, sift_like_vectors
    v = sift_like_vectors(64, 16, seed=21)
    return v, knn_graph(v, 8)


def tie_shape():
    """Integer vectors in which every vector appears twice: equal distances in
    the heap and in the final (distance, id) sort."""
    from pacmann_amd.synth import knn_graph
    v = np.repeat(np.random.default_rng(31).integers(0, 4, size=(1024, 32)).astype(np.float32), 2, axis=0)
    return v, knn_graph(v, 32)


def zero_row_shape():
    """The base shape with the neighbour lists of 5 % of the vertices zeroed
    (skipped by search.go:192-199) and id 0 placed in many other lists."""
    v, g = _base()
    g = g.copy()
    rng = np.random.default_rng(41)
    g[rng.choice(len(g), len(g) // 10, replace=False), 3] = 0
    g[rng.choice(len(g), len(g) // 20, replace=False)] = 0
    return v, g


def island_shape():
    """2,016 mainland points and an island of 32 points far away whose
    neighbour lists stay on the island: a search that starts there with
    parallel = 1 has emptied its heap after 32 pops."""
    from pacmann_amd.synth import knn_graph, sift_like_vectors
    v = sift_like_vectors(2048, 32, seed=51)
    v[2016:] += 10000.0
    return v, knn_graph(v, 16)


ISLAND_SEARCH_SEED = 3


def test_base_shape(ctx, oracle):
    v, g = _base()
    gi, og = _pair(ctx, oracle, v, g)
    _, _, dq = _same(gi, og, v[:64] + 3.0, 10, 20, 3)
    assert _oracle_drew_nothing(oracle, og, v, g)
    assert dq == 64


@pytest.mark.parametrize("d,m,par,k", [(100, 24, 3, 10), (192, 16, 8, 100)])
def test_odd_shapes(ctx, oracle, d, m, par, k):
    """d = 100: the L2's scalar tail, m no multiple of 32; d = 192, parallel 8:
    128 positions a round and a 4,096-slot state (147 KB of LDS)."""
    from pacmann_amd.synth import knn_graph, sift_like_vectors
    v = sift_like_vectors(3000, d, seed=13)
    g = knn_graph(v, m)
    gi, og = _pair(ctx, oracle, v, g)
    _, _, dq = _same(gi, og, v[100:133] + 2.0, k, 20, par)
    assert _oracle_drew_nothing(oracle, og, v, g)
    assert dq == 33


def test_ties(ctx, oracle):
    v, g = tie_shape()
    gi, og = _pair(ctx, oracle, v, g)
    qs = np.concatenate([v[:24], v[100:124] + 1.0])   # on a vector (distance 0 twice) and off it
    _, _, dq = _same(gi, og, qs, 10, 20, 3)
    assert _oracle_drew_nothing(oracle, og, v, g)
    assert dq == len(qs)


def test_zero_rows(ctx, oracle):
    v, g = zero_row_shape()
    assert not g[(g == 0).all(axis=1)].any() and ((g == 0).any(axis=1) & (g != 0).any(axis=1)).sum() > 100
    gi, og = _pair(ctx, oracle, v, g)
    _, _, dq = _same(gi, og, v[200:264] + 3.0, 10, 20, 3)
    assert _oracle_drew_nothing(oracle, og, v, g)
    assert dq == 64


def test_empty_heap_every_query(ctx, oracle):
    v, g = small_shape()
    gi, og = _pair(ctx, oracle, v, g)
    _, _, dq = _same(gi, og, v[:8] + 1.0, 10, 20, 4)
    assert dq == 0
    # the id stream ended in the same state: one more search agrees
    q = v[9] + 2.0
    a, b = gi.SearchKNN(q, 10, 20, 4), og.SearchKNN(q, 10, 20, 4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert gi.counts() == og.counts()


def test_empty_heap_some_queries(ctx, oracle):
    v, g = island_shape()
    gi, og = _pair(ctx, oracle, v, g, search_seed=ISLAND_SEARCH_SEED)
    assert (gi.GetStartVertex()[0] >= 2016).any()
    qs = v[:16] + 1.0
    qs[3::4] = v[2016:2020] + 1.0   # 12 mainland queries interleaved with 4 island queries
    _, _, dq = _same(gi, og, qs, 10, 40, 1)
    assert 0 < dq < 16


def test_edges(ctx, oracle):
    v, g = _base()
    gi, og = _pair(ctx, oracle, v, g)
    qs = v[300:310] + 3.0
    _, st, dq = _same(gi, og, qs, 10, 0, 3)   # no round: the start vertices alone
    assert dq == 10 and (st[:, :3] == 0).all() and (st[:, 3:] == -1).all()
    ids, st, dq = _same(gi, og, np.zeros((0, 128), np.float32), 10, 20, 3)
    assert dq == 0 and ids.shape == (0, 10)
    _, _, dq = _same(gi, og, qs[:3], 10, 20, 3, benchmarking=True)   # draws every id: the host's
    assert dq == 0
    # k above the known set: at most 4 + 2 x 32 known vertices after two rounds
    vs, gs = small_shape()
    gi, og = _pair(ctx, oracle, vs, gs)
    ids, st, dq = _same(gi, og, vs[:8] + 1.0, 100, 2, 4)
    assert _oracle_drew_nothing(oracle, og, vs, gs)
    assert dq == 8 and (ids[:, 64:] == -1).all() and (st[:, 64:] == -1).all() and (ids[:, :4] >= 0).all()
    # a private graph takes the sequential path
    from pacmann_amd.synth import random_graph, sift_like_vectors
    vp, gp = sift_like_vectors(2048, 32, seed=61), random_graph(2048, 16, seed=62)
    gi, og = _pair(ctx, oracle, vp, gp, nonprivate=False, pir_seed=71, search_seed=72)
    _, _, dq = _same(gi, og, vp[:3] + 1.0, 10, 5, 2)
    assert dq == 0


def test_timing(oracle):
    import pacmann_amd as pm
    c = pm.Context(0)
    c.timing(1)
    v, g = _base()
    gi, og = _pair(c, oracle, v, g)
    _, _, dq = _same(gi, og, v[:64] + 3.0, 10, 20, 3)
    n, ms, by = c.timing_get("knn_batch")
    assert dq == 64 and n >= 1 and ms > 0
    ns = int(np.sqrt(len(v)))
    assert by == n * 64 * (ns + 20 * 3 * 32) * (128 + 32) * 4
    assert c.timing_get("host_knn_batch_fallback")[0] == 0
