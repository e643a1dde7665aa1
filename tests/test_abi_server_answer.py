"""The server-role entry points (pm_batchpir_server_answer,
pm_batchpir_max_set_size) exist with their signatures in the ctypes table, and
the argument checks that need no handle answer PM_EINVAL with their text
before any HIP call (no device needed).  The checks that read a handle (stride,
partition, shard, offset) need a device to make one: they are in
tests/test_gpu_server_answer.py, with the same "out stays untouched" rule."""
import ctypes as C

import numpy as np
import pytest

PM_EINVAL = -1   # include/pacmann.h


def test_symbols_and_signatures():
    import pacmann_amd as pm
    for name in ("pm_batchpir_server_answer", "pm_batchpir_max_set_size"):
        assert name in pm.SIGNATURES and hasattr(pm.lib(), name)
    res, args = pm.SIGNATURES["pm_batchpir_server_answer"]
    assert res is C.c_int
    assert args == [pm.vp, pm.u32p, pm.u32p, pm.u64, pm.u64, pm.u64p]   # h, parts, offsets, stride, nq, out
    assert pm.SIGNATURES["pm_batchpir_max_set_size"] == (pm.u64, [pm.vp])
    fn = pm.lib().pm_batchpir_server_answer
    assert fn.restype is C.c_int and list(fn.argtypes) == args
    assert callable(pm.SimpleBatchPianoPIR.ServerAnswer)
    assert isinstance(pm.SimpleBatchPianoPIR.max_set_size, property)
    assert pm.lib().pm_batchpir_max_set_size(None) == 0


def test_header_declares_them():
    from pathlib import Path
    text = (Path(__file__).resolve().parent.parent / "include" / "pacmann.h").read_text()
    assert "int  pm_batchpir_server_answer(pm_batchpir* h, const uint32_t* parts" in text
    assert "uint64_t pm_batchpir_max_set_size(pm_batchpir* h);" in text


def test_null_arguments():
    import pacmann_amd as pm
    L = pm.lib()
    h = C.c_void_p(1)   # a non-NULL handle that no check before the HIP calls may touch
    parts = np.zeros(2, dtype=np.uint32)
    offs = np.zeros((2, 8), dtype=np.uint32)
    out = np.full((2, 4), 0xA5A5, dtype=np.uint64)
    pp, op, up = parts.ctypes.data_as(pm.u32p), offs.ctypes.data_as(pm.u32p), out.ctypes.data_as(pm.u64p)
    cases = [
        lambda: L.pm_batchpir_server_answer(None, pp, op, 8, 2, up),
        lambda: L.pm_batchpir_server_answer(h, None, op, 8, 2, up),
        lambda: L.pm_batchpir_server_answer(h, pp, None, 8, 2, up),
        lambda: L.pm_batchpir_server_answer(h, pp, op, 8, 2, None),
    ]
    for i, call in enumerate(cases):
        assert L.pm_ctx_mem_info(None, None, None) == PM_EINVAL   # another text first
        assert L.pm_last_error() == b"ctx is NULL"
        assert call() == PM_EINVAL, i
        assert L.pm_last_error().startswith(b"NULL argument"), (i, L.pm_last_error())
        assert (out == 0xA5A5).all(), i
    # nq == 0 returns 0 and touches nothing, whatever the pointers are
    assert L.pm_batchpir_server_answer(h, None, None, 0, 0, None) == 0
    assert L.pm_batchpir_server_answer(None, pp, op, 8, 0, up) == 0
    assert (out == 0xA5A5).all()


def test_wrapper_refuses_bad_arrays():
    """Before the C call: a silent cast or reshape would hide the caller's mistake."""
    import pacmann_amd as pm
    p = pm.SimpleBatchPianoPIR.__new__(pm.SimpleBatchPianoPIR)
    p.h, p.E, p._owned = None, 4, False
    with pytest.raises(TypeError, match="offsets must be uint32"):
        p.ServerAnswer([0], np.zeros((1, 8), dtype=np.int64))
    with pytest.raises(ValueError, match=r"offsets must be \[nq, stride\]"):
        p.ServerAnswer([0], np.zeros(8, dtype=np.uint32))
    with pytest.raises(ValueError, match="one partition per offset set"):
        p.ServerAnswer([0, 1], np.zeros((1, 8), dtype=np.uint32))
