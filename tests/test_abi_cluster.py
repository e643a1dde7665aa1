"""pm_kmeans and pm_cluster_* exist, refuse bad arguments with PM_EINVAL and a
text before any HIP call (no device needed), and are bound in Python."""
import ctypes as C

import numpy as np

PM_EINVAL = -1   # include/pacmann.h
NULL_TEXT = b"NULL argument"
DIM_TEXT = b"dim must be in [1, 1024]"
N_TEXT = b"n must be in [1, 2^32-1)"
NC_TEXT = b"nc must be in [1, n]"
NITER_TEXT = b"niter must be in [0, 10000]"


def test_cluster_argument_checks():
    import pacmann_amd as pm
    L = pm.lib()
    h = C.c_void_p(1)   # a non-NULL context / index that no check before the HIP calls may touch
    v = np.zeros((64, 16), dtype=np.float32)
    lab = np.zeros(64, dtype=np.uint32)
    bad = lab.copy()
    bad[63] = 4
    ids = np.zeros((1, 129), dtype=np.int64)
    out = C.c_void_p()
    fp, lp, bp, ip = (v.ctypes.data_as(pm.f32p), lab.ctypes.data_as(pm.u32p), bad.ctypes.data_as(pm.u32p),
                      ids.ctypes.data_as(pm.i64p))
    op = C.byref(out)
    km, cr, se = L.pm_kmeans, L.pm_cluster_create, L.pm_cluster_search
    cases = [
        (lambda: km(None, fp, 64, 16, 4, 1, 1, None, fp, lp, None, None), NULL_TEXT),
        (lambda: km(h, None, 64, 16, 4, 1, 1, None, fp, lp, None, None), NULL_TEXT),
        (lambda: km(h, fp, 64, 16, 4, 1, 1, None, None, lp, None, None), NULL_TEXT),
        (lambda: km(h, fp, 64, 16, 4, 1, 1, None, fp, None, None, None), NULL_TEXT),
        (lambda: km(h, fp, 64, 0, 4, 1, 1, None, fp, lp, None, None), DIM_TEXT),
        (lambda: km(h, fp, 64, 1025, 4, 1, 1, None, fp, lp, None, None), DIM_TEXT),
        (lambda: km(h, fp, 64, 2 ** 32 + 16, 4, 1, 1, None, fp, lp, None, None), DIM_TEXT),
        (lambda: km(h, fp, 0, 16, 4, 1, 1, None, fp, lp, None, None), N_TEXT),
        (lambda: km(h, fp, 2 ** 32 - 1, 16, 4, 1, 1, None, fp, lp, None, None), N_TEXT),
        (lambda: km(h, fp, 64, 16, 0, 1, 1, None, fp, lp, None, None), NC_TEXT),
        (lambda: km(h, fp, 64, 16, 65, 1, 1, None, fp, lp, None, None), NC_TEXT),
        (lambda: km(h, fp, 64, 16, 4, 10001, 1, None, fp, lp, None, None), NITER_TEXT),
        (lambda: cr(None, fp, 64, 16, fp, 4, lp, op), NULL_TEXT),
        (lambda: cr(h, None, 64, 16, fp, 4, lp, op), NULL_TEXT),
        (lambda: cr(h, fp, 64, 16, None, 4, lp, op), NULL_TEXT),
        (lambda: cr(h, fp, 64, 16, fp, 4, None, op), NULL_TEXT),
        (lambda: cr(h, fp, 64, 16, fp, 4, lp, None), NULL_TEXT),
        (lambda: cr(h, fp, 64, 0, fp, 4, lp, op), DIM_TEXT),
        (lambda: cr(h, fp, 64, 1025, fp, 4, lp, op), DIM_TEXT),
        (lambda: cr(h, fp, 0, 16, fp, 4, lp, op), N_TEXT),
        (lambda: cr(h, fp, 2 ** 32 - 1, 16, fp, 4, lp, op), N_TEXT),
        (lambda: cr(h, fp, 64, 16, fp, 0, lp, op), b"nc must be in [1, 2^32-1)"),
        (lambda: cr(h, fp, 64, 16, fp, 4, bp, op), b"label out of range"),
        (lambda: cr(h, fp, 64, 16, fp, 1, bp, op), b"label out of range"),
        (lambda: se(None, fp, 1, 10, 1, ip, None, None, None), NULL_TEXT),
        (lambda: se(h, None, 1, 10, 1, ip, None, None, None), NULL_TEXT),
        (lambda: se(h, fp, 1, 10, 1, None, None, None, None), NULL_TEXT),
        (lambda: se(h, fp, 1, 0, 1, ip, None, None, None), b"k must be in [1, 128]"),
        (lambda: se(h, fp, 1, 129, 1, ip, None, None, None), b"k must be in [1, 128]"),
        (lambda: se(h, fp, 0, 10, 1, ip, None, None, None), b"nq must be > 0"),
        (lambda: L.pm_cluster_info(None, None, None, None, None, None), NULL_TEXT),
    ]
    for i, (call, want) in enumerate(cases):
        assert L.pm_ctx_mem_info(None, None, None) == PM_EINVAL   # another text first
        assert L.pm_last_error() == b"ctx is NULL"
        assert call() == PM_EINVAL, i
        assert L.pm_last_error().startswith(want), (i, L.pm_last_error())
    assert out.value is None
    L.pm_cluster_destroy(None)   # a no-op


def test_cluster_bindings_exist():
    import pacmann_amd as pm
    for name in ("pm_kmeans", "pm_cluster_create", "pm_cluster_destroy", "pm_cluster_info", "pm_cluster_search"):
        assert name in pm.SIGNATURES and hasattr(pm.lib(), name)
    assert callable(pm.kmeans)
    for name in ("train", "load", "save", "search", "close"):
        assert callable(getattr(pm.ClusterIndex, name))


def test_wrapper_refuses_bad_labels_before_any_context():
    import pacmann_amd as pm
    import pytest

    class NoCtx:   # stands in for a context: the checks below come before its first use
        h = None
    v = np.zeros((8, 4), np.float32)
    cen = np.zeros((2, 4), np.float32)
    with pytest.raises(TypeError, match="labels must be integers"):
        pm.ClusterIndex(v, cen, np.zeros(8, np.float32), NoCtx())
    with pytest.raises(ValueError, match="labels have the wrong shape"):
        pm.ClusterIndex(v, cen, np.zeros(7, np.int64), NoCtx())
    with pytest.raises(ValueError, match="centroids have the wrong shape"):
        pm.ClusterIndex(v, np.zeros((2, 5), np.float32), np.zeros(8, np.int64), NoCtx())
    with pytest.raises(ValueError, match="label out of range"):
        pm.ClusterIndex(v, cen, np.full(8, -1, np.int64), NoCtx())
