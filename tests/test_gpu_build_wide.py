"""pm_build_graph_wide against oracle.build_graph row for row: the wide kNN
candidates (K = int(1.5 m) + self), k_prune<false> in both passes and the host's
edge work, at rows of 200 to 960 dimensions."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def rows(n, dim, integer, seed):
    rng = np.random.default_rng([seed, n, dim])
    if integer:
        return rng.integers(0, 256, (n, dim)).astype(np.float32)
    c = rng.standard_normal((10, dim)).astype(np.float32)
    return (c[np.arange(n) % 10] + 0.3 * rng.standard_normal((n, dim))).astype(np.float32)


@pytest.mark.parametrize("n,dim,m,integer", [(300, 200, 8, False), (300, 960, 32, False), (200, 384, 8, True),
                                             (9, 256, 8, False)],
                         ids=["d200_m8", "d960_m32_K48", "d384_m8_integers", "n_is_m_plus_1"])
def test_build_graph_wide_equals_oracle(ctx, oracle, n, dim, m, integer):
    import pacmann_amd as pm
    v = rows(n, dim, integer, seed=m)
    g, t = pm.build_graph_wide(v, m, 1.2, seed=9, ctx=ctx)
    o = oracle.build_graph(v, m, 1.2, seed=9)
    print(f"n={n} d={dim} m={m}: knn_fallback_rows {t['knn_fallback_rows']}")
    if not np.array_equal(g, o):
        bad = np.where((g != o).any(axis=1))[0]
        pytest.fail(f"{len(bad)} rows differ, first {bad[:5].tolist()}: {g[bad[0]].tolist()} vs {o[bad[0]].tolist()}")
    assert (g != np.arange(n, dtype=np.uint32)[:, None]).all()
    assert 0 <= t["knn_fallback_rows"] <= n
    times = [t["knn_s"], t["prune1_s"], t["host_edges_s"], t["prune2_s"]]
    assert len(times) == 4 and all(x >= 0 for x in times)
