"""The grouped GetVertexInfo entry points (pm_graph_group_*) exist with the
declared signatures and refuse bad arguments with PM_EINVAL and a text.  The
refusals that read nothing through a session pointer need no device; the
others need real sessions and are marked gpu."""
import ctypes as C

import numpy as np
import pytest

PM_EINVAL = -1   # include/pacmann.h


def _refused(L, call, want):
    assert L.pm_ctx_mem_info(None, None, None) == PM_EINVAL   # another text first
    assert L.pm_last_error() == b"ctx is NULL"
    assert call() == PM_EINVAL
    assert want in L.pm_last_error(), L.pm_last_error()


def test_symbols_and_signatures():
    import pacmann_amd as pm
    L = pm.lib()
    vp, u64p, f32p, u32p, u8p = pm.vp, pm.u64p, pm.f32p, pm.u32p, pm.u8p
    want = {
        "pm_graph_group_create": (C.c_int, [C.POINTER(vp), C.c_uint32, C.POINTER(vp)]),
        "pm_graph_group_destroy": (None, [vp]),
        "pm_graph_group_get_vertex_info": (C.c_int, [vp, u64p, u64p, f32p, u32p, u8p, f32p, f32p]),
        "pm_graph_group_preprocess": (C.c_int, [vp]),
    }
    for name, (res, args) in want.items():
        assert hasattr(L, name), name
        assert pm.SIGNATURES[name] == (res, args), name
        f = getattr(L, name)
        assert f.restype == res and list(f.argtypes) == args, name
    header = (pm.LIB_PATH.parent.parent / "include" / "pacmann.h").read_text()
    for name in want:
        assert name + "(" in header, name
    assert callable(pm.PIRGraphGroup) and "PIRGraphGroup" in pm.__all__
    for name in ("get_vertex_info", "preprocess"):
        assert callable(getattr(pm.PIRGraphGroup, name))


def test_refusals_without_a_device():
    import pacmann_amd as pm
    L = pm.lib()
    h = pm.vp(1)   # a non-NULL handle that no check before the refusal may read through
    out = pm.vp()
    two = (pm.vp * 2)(h, h)
    nul = (pm.vp * 2)(h, None)
    offs = np.zeros(3, dtype=np.uint64)
    d = np.zeros(4, dtype=np.float32)
    op, dp = offs.ctypes.data_as(pm.u64p), d.ctypes.data_as(pm.f32p)
    _refused(L, lambda: L.pm_graph_group_create(None, 2, C.byref(out)), b"NULL argument")
    _refused(L, lambda: L.pm_graph_group_create(two, 2, None), b"NULL argument")
    _refused(L, lambda: L.pm_graph_group_create(two, 0, C.byref(out)), b"NULL argument")   # S = 0
    _refused(L, lambda: L.pm_graph_group_create(nul, 2, C.byref(out)), b"NULL session")
    _refused(L, lambda: L.pm_graph_group_create(two, 2, C.byref(out)), b"a session appears twice")
    _refused(L, lambda: L.pm_graph_group_get_vertex_info(None, None, op, None, None, None, None, None), b"NULL argument")
    _refused(L, lambda: L.pm_graph_group_get_vertex_info(h, None, None, None, None, None, None, None), b"NULL argument")
    _refused(L, lambda: L.pm_graph_group_get_vertex_info(h, None, op, None, None, None, None, dp), b"dist needs the queries")
    _refused(L, lambda: L.pm_graph_group_preprocess(None), b"NULL argument")
    assert not out.value
    L.pm_graph_group_destroy(None)


@pytest.mark.gpu
def test_refusals_of_real_sessions(ctx):
    import pacmann_amd as pm
    from pacmann_amd.synth import random_graph, sift_like_vectors
    n, dim, m = 2_000, 16, 8
    v, g = sift_like_vectors(n, dim, seed=3), random_graph(n, m, seed=4)
    base = pm.PIRGraphInfo(v, g, pir_seed=1, search_seed=2, ctx=pm.Context(0))
    with pytest.raises(RuntimeError, match="session 0 is not preprocessed"):
        pm.PIRGraphGroup([base])
    base.Preprocess()
    sess = base.Session(5, 6)
    with pytest.raises(RuntimeError, match="session 1 is not preprocessed"):
        pm.PIRGraphGroup([base, sess])
    sess.Preprocess()
    plain = pm.PIRGraphInfo(v, g, nonprivate=True, pir_seed=1, search_seed=2, ctx=pm.Context(0))
    plain.Preprocess()
    with pytest.raises(RuntimeError, match="session 1 is not private"):
        pm.PIRGraphGroup([base, plain])
    with pytest.raises(RuntimeError, match="a session appears twice"):
        pm.PIRGraphGroup([base, sess, base])
    other = pm.PIRGraphInfo(v, g, pir_seed=1, search_seed=2, ctx=pm.Context(0))
    other.Preprocess()
    with pytest.raises(RuntimeError, match="clients of one server DB"):
        pm.PIRGraphGroup([base, other])
    twin = base.Session(7, 8, ctx=sess.ctx)
    twin.Preprocess()
    with pytest.raises(RuntimeError, match="distinct contexts"):
        pm.PIRGraphGroup([base, sess, twin])
    grp = pm.PIRGraphGroup([base, sess])
    before = [s.counts() for s in (base, sess)]
    with pytest.raises(RuntimeError, match="session 1: vertex id 2000 out of range"):
        grp.get_vertex_info([[1, 2, 3, 4], [5, n]])
    offs = np.array([0, 4, 2], dtype=np.uint64)
    ids = np.arange(4, dtype=np.uint64)
    assert pm.lib().pm_graph_group_get_vertex_info(grp.h, ids.ctypes.data_as(pm.u64p), offs.ctypes.data_as(pm.u64p),
                                                   None, None, None, None, None) == PM_EINVAL
    assert b"offs descends at session 1" in pm.lib().pm_last_error()
    assert [s.counts() for s in (base, sess)] == before   # nobody's state moved
