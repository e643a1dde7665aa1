"""The 128-key entry points (pm_knn_k128, pm_build_graph_k128,
pm_knn_stages_k128, pm_knn_k128_top) refuse bad arguments with PM_EINVAL and a
text before any HIP call (no device needed), and tests/knn_k128_ref.py's
generators keep what they promise."""
import ctypes as C

import numpy as np

from tests import knn_k128_ref as K

PM_EINVAL = -1   # include/pacmann.h
DIM_TEXT = b"dim must be in [1, 1024]"
K_TEXT = b"k must be in [1, 128]"
M_TEXT = b"m must be in [1, 64]"
N_TEXT = b"n must be in [1, 2^32-1)"


def test_k128_argument_checks():
    import pacmann_amd as pm
    L = pm.lib()
    h = C.c_void_p(1)   # a non-NULL context that no check before the HIP calls may touch
    v = np.zeros((64, 16), dtype=np.float32)
    ids = np.zeros((1, 129), dtype=np.int64)
    g = np.zeros((64, 65), dtype=np.uint32)
    fb = C.c_uint64(7)
    vp, ip, gp = v.ctypes.data_as(pm.f32p), ids.ctypes.data_as(pm.i64p), g.ctypes.data_as(pm.u32p)
    cand, pref = np.zeros((1, 128), np.uint32), np.zeros((1, 128), np.float32)
    o = pm.KnnStagesOut()
    o.cand, o.pref = cand.ctypes.data_as(pm.u32p), pref.ctypes.data_as(pm.f32p)
    empty = pm.KnnStagesOut()
    cases = [
        (lambda: L.pm_knn_k128(None, vp, 64, 16, vp, 1, 10, ip, None, C.byref(fb)), b"NULL argument"),
        (lambda: L.pm_knn_k128(h, None, 64, 16, vp, 1, 10, ip, None, C.byref(fb)), b"NULL argument"),
        (lambda: L.pm_knn_k128(h, vp, 64, 16, None, 1, 10, ip, None, C.byref(fb)), b"NULL argument"),
        (lambda: L.pm_knn_k128(h, vp, 64, 16, vp, 1, 10, None, None, C.byref(fb)), b"NULL argument"),
        (lambda: L.pm_knn_k128(h, vp, 64, 0, vp, 1, 10, ip, None, C.byref(fb)), DIM_TEXT),
        (lambda: L.pm_knn_k128(h, vp, 64, 1025, vp, 1, 10, ip, None, C.byref(fb)), DIM_TEXT),
        (lambda: L.pm_knn_k128(h, vp, 64, 16, vp, 1, 0, ip, None, C.byref(fb)), K_TEXT),
        (lambda: L.pm_knn_k128(h, vp, 64, 16, vp, 1, 129, ip, None, C.byref(fb)), K_TEXT),
        (lambda: L.pm_knn_k128(h, vp, 0, 16, vp, 1, 10, ip, None, C.byref(fb)), N_TEXT),
        (lambda: L.pm_knn_k128(h, vp, 2 ** 32 - 1, 16, vp, 1, 10, ip, None, C.byref(fb)), N_TEXT),
        (lambda: L.pm_build_graph_k128(None, vp, 64, 16, 8, 1.2, 1, gp, None, C.byref(fb)), b"NULL argument"),
        (lambda: L.pm_build_graph_k128(h, None, 64, 16, 8, 1.2, 1, gp, None, C.byref(fb)), b"NULL argument"),
        (lambda: L.pm_build_graph_k128(h, vp, 64, 16, 8, 1.2, 1, None, None, C.byref(fb)), b"NULL argument"),
        (lambda: L.pm_build_graph_k128(h, vp, 64, 0, 8, 1.2, 1, gp, None, C.byref(fb)), DIM_TEXT),
        (lambda: L.pm_build_graph_k128(h, vp, 64, 1025, 8, 1.2, 1, gp, None, C.byref(fb)), DIM_TEXT),
        (lambda: L.pm_build_graph_k128(h, vp, 64, 16, 0, 1.2, 1, gp, None, C.byref(fb)), M_TEXT),
        (lambda: L.pm_build_graph_k128(h, vp, 64, 16, 65, 1.2, 1, gp, None, C.byref(fb)), M_TEXT),
        (lambda: L.pm_build_graph_k128(h, vp, 64, 16, 64, 1.2, 1, gp, None, C.byref(fb)), b"n must be > m"),
        (lambda: L.pm_knn_stages_k128(None, vp, 64, 16, vp, 1, 10, C.byref(o)), b"NULL argument"),
        (lambda: L.pm_knn_stages_k128(h, vp, 64, 16, vp, 1, 10, None), b"NULL argument"),
        (lambda: L.pm_knn_stages_k128(h, vp, 64, 16, vp, 1, 10, C.byref(empty)), b"NULL argument"),
        (lambda: L.pm_knn_stages_k128(h, vp, 64, 0, vp, 1, 10, C.byref(o)), DIM_TEXT),
        (lambda: L.pm_knn_stages_k128(h, vp, 64, 1025, vp, 1, 10, C.byref(o)), DIM_TEXT),
        (lambda: L.pm_knn_stages_k128(h, vp, 64, 16, vp, 1, 0, C.byref(o)), K_TEXT),
        (lambda: L.pm_knn_stages_k128(h, vp, 64, 16, vp, 1, 129, C.byref(o)), K_TEXT),
        (lambda: L.pm_knn_stages_k128(h, vp, 0, 16, vp, 1, 10, C.byref(o)), N_TEXT),
    ]
    for i, (call, want) in enumerate(cases):
        assert L.pm_ctx_mem_info(None, None, None) == PM_EINVAL   # another text first
        assert L.pm_last_error() == b"ctx is NULL"
        assert call() == PM_EINVAL, i
        assert L.pm_last_error().startswith(want), (i, L.pm_last_error())
    assert fb.value in (0, 7)   # zeroed only by a call that got past its NULL check


def test_k128_bindings_exist():
    import pacmann_amd as pm
    for name in ("knn_k128", "knn_stages_k128", "build_graph_k128"):
        assert callable(getattr(pm, name))
    for name in ("pm_knn_k128", "pm_build_graph_k128", "pm_knn_stages_k128", "pm_knn_k128_top"):
        assert name in pm.SIGNATURES and hasattr(pm.lib(), name)
    assert pm.lib().pm_knn_k128_top() == 128 == K.TOP


def test_shape_cases_cover_every_axis_twice():
    cases = K.shape_cases()
    assert 28 <= len(cases) <= 34
    for axis, values in ((0, K.SHAPE_N), (1, K.SHAPE_NQ), (2, K.SHAPE_DIM)):
        for x in values:
            assert sum(c[axis] == x for c in cases) >= 2, (axis, x)
    for k in (1, 64, 65, 100, 127, 128):
        assert sum(c[3] == k for c in cases) >= 2, k
    assert sum(c[3] == c[0] + 1 for c in cases) >= 2       # k = n + 1
    assert sum(c[3] > c[0] for c in cases) >= 4            # padding beyond n
    for d in K.SHAPE_DIM:
        assert {c[4] for c in cases if c[2] == d} == {False, True}, d
    assert all(1 <= c[3] <= K.TOP for c in cases)


def test_identical_rows_tie_beyond_128():
    for dim in (100, 200):
        v, q, ntie = K.identical_rows(dim)
        same = (v[None, :, :] == q[:ntie, None, :]).all(axis=2)
        assert (same.sum(axis=1) == 300).all() and same[0, 10:138].all() and not same[0, :10].any()
        other = (v[None, :, :] == q[ntie:, None, :]).all(axis=2)
        assert (other.sum(axis=1) == 1).all()


def test_near_tie_rows_make_the_subset_strict(oracle):
    """At k = 48 the float64 verdict leaves the near-duplicate queries uncertified
    with 64 keys and certified with 128, for both dims; the other queries are
    certified either way by a wide margin."""
    for dim in (100, 320):
        v, q, ntie = K.near_tie_rows(dim)
        assert 64 < K.NEAR_DUP < K.TOP and len(np.unique(v[:K.NEAR_DUP], axis=0)) == K.NEAR_DUP
        sure64, sure128 = K.subset_verdict(oracle, v, q, 48)
        assert sure64[:ntie].all() and sure128[:ntie].all(), dim
        assert sure128.all() and not sure64[ntie:].any()
