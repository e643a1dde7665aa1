"""pm_build_graph_u8 against the oracle's graph of the rows as floats, row for
row: candidates from the int8 kNN (k_knn_i8, self dropped), the unchanged
robustPrune stages over the device's f32 copy (k_u8_to_f32); and against
pm_build_graph_k128 on clustered bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32


def build_timed(ctx, v, m):
    import pacmann_amd as pm
    names = ("u8_bias", "u8_to_f32", "knn_prefilter_u8", "to_bf16", "knn_rerank", "knn_brute")
    ctx.timing(1)
    try:
        ctx.timing_reset()
        g, t = pm.build_graph_u8(v, m, 1.2, 1, ctx)
        runs = {name: ctx.timing_get(name)[0] for name in names}
    finally:
        ctx.timing(0)
    return g, t, runs


def check_times(t):
    assert sorted(t) == ["host_edges_s", "knn_s", "prune1_s", "prune2_s"]
    assert all(x >= 0 for x in t.values())


@pytest.mark.parametrize("n,dim,m", [(300, 8, 8), (500, 128, 32), (400, 256, 64), (70, 16, 64)])
def test_equals_the_oracle(ctx, oracle, n, dim, m):
    """Narrow rows with many ties (dim 8), the SIFT width, the widest row at the
    largest m (K = 96 of 128 keys) and K above n (n = 70, m = 64)."""
    v = np.random.default_rng([51, n, dim]).integers(0, 256, (n, dim), dtype=np.uint8)
    g, t, runs = build_timed(ctx, v, m)
    assert np.array_equal(g, oracle.build_graph(v.astype(F32), m, 1.2, 1))
    check_times(t)
    assert runs == {"u8_bias": 1, "u8_to_f32": 1, "knn_prefilter_u8": 1, "to_bf16": 0, "knn_rerank": 0, "knn_brute": 0}


@pytest.mark.parametrize("m", [32, 43])
def test_clustered_bytes_equal_the_float_build(ctx, oracle, m):
    import pacmann_amd as pm
    from pacmann_amd.synth import clustered_vectors
    f = clustered_vectors(1000, 128, seed=7)
    v = f.astype(np.uint8)
    assert np.array_equal(v.astype(F32), f)
    g, t, _ = build_timed(ctx, v, m)
    gf, _ = pm.build_graph_k128(f, m, 1.2, 1, ctx)
    assert np.array_equal(g, gf) and np.array_equal(g, oracle.build_graph(f, m, 1.2, 1))
    check_times(t)
