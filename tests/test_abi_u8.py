"""The uint8 entry points (pm_knn_u8, pm_build_graph_u8, pm_knn_u8_max_dim)
exist, refuse bad arguments with PM_EINVAL and a text before any HIP call (no
device needed), and their Python wrappers refuse arrays that are not uint8."""
import ctypes as C

import numpy as np
import pytest

PM_EINVAL = -1   # include/pacmann.h
DIM_TEXT = b"dim must be in [1, 256]"
K_TEXT = b"k must be in [1, 128]"
M_TEXT = b"m must be in [1, 64]"
N_TEXT = b"n must be in [1, 2^32-1)"


def test_u8_argument_checks():
    import pacmann_amd as pm
    L = pm.lib()
    h = C.c_void_p(1)   # a non-NULL context that no check before the HIP calls may touch
    v = np.zeros((66, 16), dtype=np.uint8)
    ids = np.zeros((1, 129), dtype=np.int64)
    g = np.zeros((66, 65), dtype=np.uint32)
    vp, ip, gp = v.ctypes.data_as(pm.u8p), ids.ctypes.data_as(pm.i64p), g.ctypes.data_as(pm.u32p)
    cases = [
        (lambda: L.pm_knn_u8(None, vp, 64, 16, vp, 1, 10, ip, None), b"NULL argument"),
        (lambda: L.pm_knn_u8(h, None, 64, 16, vp, 1, 10, ip, None), b"NULL argument"),
        (lambda: L.pm_knn_u8(h, vp, 64, 16, None, 1, 10, ip, None), b"NULL argument"),
        (lambda: L.pm_knn_u8(h, vp, 64, 16, vp, 1, 10, None, None), b"NULL argument"),
        (lambda: L.pm_knn_u8(h, vp, 64, 0, vp, 1, 10, ip, None), DIM_TEXT),
        (lambda: L.pm_knn_u8(h, vp, 64, 257, vp, 1, 10, ip, None), DIM_TEXT),
        (lambda: L.pm_knn_u8(h, vp, 64, 2 ** 32 + 16, vp, 1, 10, ip, None), DIM_TEXT),
        (lambda: L.pm_knn_u8(h, vp, 64, 16, vp, 1, 0, ip, None), K_TEXT),
        (lambda: L.pm_knn_u8(h, vp, 64, 16, vp, 1, 129, ip, None), K_TEXT),
        (lambda: L.pm_knn_u8(h, vp, 0, 16, vp, 1, 10, ip, None), N_TEXT),
        (lambda: L.pm_knn_u8(h, vp, 2 ** 32 - 1, 16, vp, 1, 10, ip, None), N_TEXT),
        (lambda: L.pm_build_graph_u8(None, vp, 66, 16, 8, 1.2, 1, gp, None), b"NULL argument"),
        (lambda: L.pm_build_graph_u8(h, None, 66, 16, 8, 1.2, 1, gp, None), b"NULL argument"),
        (lambda: L.pm_build_graph_u8(h, vp, 66, 16, 8, 1.2, 1, None, None), b"NULL argument"),
        (lambda: L.pm_build_graph_u8(h, vp, 66, 0, 8, 1.2, 1, gp, None), DIM_TEXT),
        (lambda: L.pm_build_graph_u8(h, vp, 66, 257, 8, 1.2, 1, gp, None), DIM_TEXT),
        (lambda: L.pm_build_graph_u8(h, vp, 66, 16, 0, 1.2, 1, gp, None), M_TEXT),
        (lambda: L.pm_build_graph_u8(h, vp, 66, 16, 65, 1.2, 1, gp, None), M_TEXT),
        (lambda: L.pm_build_graph_u8(h, vp, 64, 16, 64, 1.2, 1, gp, None), b"n must be > m"),
        (lambda: L.pm_build_graph_u8(h, vp, 8, 16, 8, 1.2, 1, gp, None), b"n must be > m"),
        (lambda: L.pm_build_graph_u8(h, vp, 2 ** 32 - 1, 16, 8, 1.2, 1, gp, None), b"n must be > m"),
    ]
    for i, (call, want) in enumerate(cases):
        assert L.pm_ctx_mem_info(None, None, None) == PM_EINVAL   # another text first
        assert L.pm_last_error() == b"ctx is NULL"
        assert call() == PM_EINVAL, i
        assert L.pm_last_error().startswith(want), (i, L.pm_last_error())


def test_u8_bindings_exist():
    import pacmann_amd as pm
    from pacmann_amd import loader
    for name in ("knn_u8", "build_graph_u8", "knn_u8_max_dim"):
        assert callable(getattr(pm, name))
    for name in ("pm_knn_u8", "pm_build_graph_u8", "pm_knn_u8_max_dim"):
        assert name in pm.SIGNATURES and hasattr(pm.lib(), name)
    assert pm.lib().pm_knn_u8_max_dim() == 256 == pm.knn_u8_max_dim()
    assert "load_bvecs_u8" in loader.__all__


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int8, np.int32])
def test_wrappers_refuse_other_dtypes(dtype):
    """Before any context is made: a silent cast would hide the caller's mistake."""
    import pacmann_amd as pm
    good = np.zeros((70, 16), np.uint8)
    bad = np.zeros((70, 16), dtype)
    with pytest.raises(TypeError, match="base must be uint8"):
        pm.knn_u8(bad, good, 5)
    with pytest.raises(TypeError, match="queries must be uint8"):
        pm.knn_u8(good, bad, 5)
    with pytest.raises(TypeError, match="vectors must be uint8"):
        pm.build_graph_u8(bad, 8)
