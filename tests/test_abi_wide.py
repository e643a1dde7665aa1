"""The four wide entry points (pm_knn_wide, pm_build_graph_wide,
pm_knn_stages_wide, pm_robust_prune_wide) refuse bad arguments with PM_EINVAL
and a text before any HIP call (no device needed), and tests/knn_wide_ref.py's
padding rule and c_dp against hand-computed numbers."""
import ctypes as C

import numpy as np

from tests import knn_wide_ref as W

PM_EINVAL = -1   # include/pacmann.h
DIM_TEXT = b"dim must be in [1, 1024]"


def test_wide_argument_checks():
    import pacmann_amd as pm
    L = pm.lib()
    h = C.c_void_p(1)   # a non-NULL context that no check before the HIP calls may touch
    v = np.zeros((64, 16), dtype=np.float32)
    ids = np.zeros((1, 65), dtype=np.int64)
    g = np.zeros((64, 43), dtype=np.uint32)
    fb = C.c_uint64(7)
    vp, ip, gp = v.ctypes.data_as(pm.f32p), ids.ctypes.data_as(pm.i64p), g.ctypes.data_as(pm.u32p)
    cand, pref = np.zeros((1, 64), np.uint32), np.zeros((1, 64), np.float32)
    o = pm.KnnStagesOut()
    o.cand, o.pref = cand.ctypes.data_as(pm.u32p), pref.ctypes.data_as(pm.f32p)
    empty = pm.KnnStagesOut()
    verts = np.array([1, 2], np.uint32)
    offs, lens = np.array([0, 2], np.uint64), np.array([2, 2], np.uint32)
    pid = np.array([3, 4, 5, 6], np.uint32)
    out, ol, err = np.zeros((2, 64), np.uint32), np.zeros(2, np.uint32), np.zeros(1, np.uint32)
    u32, u64 = (lambda a: a.ctypes.data_as(pm.u32p)), (lambda a: a.ctypes.data_as(pm.u64p))

    def prune(ctxh=h, X=vp, dim=8, m=4, o_=out):
        return L.pm_robust_prune_wide(ctxh, X, 10, dim, u32(verts), 2, u64(offs), u32(lens), u32(pid), 4, m, 1.2, 0,
                                      u32(o_) if o_ is not None else None, u32(ol), u32(err))
    cases = [
        (lambda: L.pm_knn_wide(None, vp, 64, 16, vp, 1, 10, ip, None, C.byref(fb)), b"NULL argument"),
        (lambda: L.pm_knn_wide(h, None, 64, 16, vp, 1, 10, ip, None, C.byref(fb)), b"NULL argument"),
        (lambda: L.pm_knn_wide(h, vp, 64, 16, vp, 1, 10, None, None, C.byref(fb)), b"NULL argument"),
        (lambda: L.pm_knn_wide(h, vp, 64, 0, vp, 1, 10, ip, None, C.byref(fb)), DIM_TEXT),
        (lambda: L.pm_knn_wide(h, vp, 64, 1025, vp, 1, 10, ip, None, C.byref(fb)), DIM_TEXT),
        (lambda: L.pm_knn_wide(h, vp, 64, 16, vp, 1, 0, ip, None, C.byref(fb)), b"k must be in [1, 64]"),
        (lambda: L.pm_knn_wide(h, vp, 64, 16, vp, 1, 65, ip, None, C.byref(fb)), b"k must be in [1, 64]"),
        (lambda: L.pm_build_graph_wide(None, vp, 64, 16, 8, 1.2, 1, gp, None, C.byref(fb)), b"NULL argument"),
        (lambda: L.pm_build_graph_wide(h, vp, 64, 16, 8, 1.2, 1, None, None, C.byref(fb)), b"NULL argument"),
        (lambda: L.pm_build_graph_wide(h, vp, 64, 0, 8, 1.2, 1, gp, None, C.byref(fb)), DIM_TEXT),
        (lambda: L.pm_build_graph_wide(h, vp, 64, 1025, 8, 1.2, 1, gp, None, C.byref(fb)), DIM_TEXT),
        (lambda: L.pm_build_graph_wide(h, vp, 64, 16, 43, 1.2, 1, gp, None, C.byref(fb)), b"m must be in [1, 42]"),
        (lambda: L.pm_knn_stages_wide(None, vp, 64, 16, vp, 1, 10, C.byref(o)), b"NULL argument"),
        (lambda: L.pm_knn_stages_wide(h, vp, 64, 16, vp, 1, 10, None), b"NULL argument"),
        (lambda: L.pm_knn_stages_wide(h, vp, 64, 16, vp, 1, 10, C.byref(empty)), b"NULL argument"),
        (lambda: L.pm_knn_stages_wide(h, vp, 64, 0, vp, 1, 10, C.byref(o)), DIM_TEXT),
        (lambda: L.pm_knn_stages_wide(h, vp, 64, 1025, vp, 1, 10, C.byref(o)), DIM_TEXT),
        (lambda: L.pm_knn_stages_wide(h, vp, 64, 16, vp, 1, 0, C.byref(o)), b"k must be in [1, 64]"),
        (lambda: L.pm_knn_stages_wide(h, vp, 64, 16, vp, 1, 65, C.byref(o)), b"k must be in [1, 64]"),
        (lambda: prune(ctxh=None), b"NULL argument"),
        (lambda: prune(X=None), b"NULL argument"),
        (lambda: prune(o_=None), b"NULL argument"),
        (lambda: prune(dim=0), DIM_TEXT),
        (lambda: prune(dim=1025), DIM_TEXT),
        (lambda: prune(m=0), b"m must be in [1, 64]"),
        (lambda: prune(m=65), b"m must be in [1, 64]"),
    ]
    for i, (call, want) in enumerate(cases):
        assert L.pm_ctx_mem_info(None, None, None) == PM_EINVAL   # another text first
        assert L.pm_last_error() == b"ctx is NULL"
        assert call() == PM_EINVAL, i
        assert L.pm_last_error().startswith(want), (i, L.pm_last_error())
    assert fb.value in (0, 7)   # zeroed only by a call that got past its NULL check


def test_wide_bindings_exist():
    import pacmann_amd as pm
    for name in ("knn_wide", "knn_stages_wide", "robust_prune_wide", "build_graph_wide"):
        assert callable(getattr(pm, name))
    for name in ("pm_knn_wide", "pm_build_graph_wide", "pm_knn_stages_wide", "pm_robust_prune_wide"):
        assert name in pm.SIGNATURES and hasattr(pm.lib(), name)


def test_padding_rule():
    want = {1: 128, 128: 128, 129: 192, 192: 192, 193: 256, 255: 256, 256: 256, 257: 320, 320: 320, 511: 512,
            512: 512, 513: 576, 960: 960, 961: 1024, 1023: 1024, 1024: 1024}
    for dim, dp in want.items():
        assert W.pad_dim(dim) == dp, dim
    for dim in range(193, 1025):
        dp = W.pad_dim(dim)
        assert dp % 64 == 0 and dim <= dp < dim + 64


def test_c_dp_values():
    """c_dp = 2 (3 dp + 8) 2^-23 + 2^-16 (1 + 2^-6) + 2^-17 = (6 dp + 16 + 128 + 2 + 64) 2^-23 = (6 dp + 210) 2^-23."""
    for dp, num in ((256, 1746), (512, 3282), (1024, 6354)):
        assert 6 * dp + 210 == num
        assert W.c_dp(dp) == num / 2.0 ** 23
    assert abs(W.c_dp(256) - 2.081e-4) < 1e-7
    assert abs(W.c_dp(512) - 3.912e-4) < 1e-7
    assert abs(W.c_dp(1024) - 7.575e-4) < 1e-7
    assert W.c_dp(1024) > 2.0 ** -12 > W.c_dp(256)   # above the narrow path's contract from dp 320 on
    assert W.eps_bound(1024, 1.0, 2.0) == 3 * W.c_dp(1024) + 2.0 ** -50


def test_reference_shapes():
    """The restated split and norm at a wide dp: shapes, padding and one value."""
    x = np.zeros((2, 257), np.float32)
    x[0, 256] = 3.0
    x[1, :] = 1.0
    hi, lo = W.split_rows(x)
    assert hi.shape == lo.shape == (2, 320) and hi[0, 256] == 0x4040 and not lo.any() and not hi[:, 257:].any()
    assert W.norms_fixed_order(x).tolist() == [9.0, 257.0]
    cases = W.shape_cases()
    assert len(cases) == 20
    for d in W.SHAPE_DIM:
        assert sum(c[2] == d for c in cases) >= 2 and {c[4] for c in cases if c[2] == d} == {False, True}
    for p in W.SHAPE_NNQ:
        assert sum(c[:2] == p for c in cases) >= 2
    assert {c[3] for c in cases} >= {1, 64, W.K_MID}
