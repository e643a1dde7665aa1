"""The client-role entry points (pm_batchpir_client_max_sets, pm_batchpir_client_begin,
pm_batchpir_client_finish) exist with their prototypes in the header, the ctypes
table and the library, and the Python wrappers refuse a malformed answers array
before they call the library (no device needed).  What needs a handle is in
tests/test_gpu_split_query.py."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

PM_EINVAL = -1   # include/pacmann.h


def test_symbols_and_signatures():
    import pacmann_amd as pm
    u8p = C.POINTER(C.c_uint8)
    want = {
        "pm_batchpir_client_max_sets": (pm.u64, [pm.vp, pm.u64]),                                   # h, n
        "pm_batchpir_client_begin": (C.c_int, [pm.vp, pm.u64p, pm.u64, pm.u32p, pm.u32p, pm.u64, pm.u64, pm.u64p]),
        "pm_batchpir_client_finish": (C.c_int, [pm.vp, pm.u64p, pm.u64, pm.u64p, u8p]),             # h, answers, nq, out, ok
    }
    for name, (res, args) in want.items():
        assert name in pm.SIGNATURES and hasattr(pm.lib(), name), name
        assert pm.SIGNATURES[name] == (res, args), name
        fn = getattr(pm.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert callable(pm.SimpleBatchPianoPIR.QueryBegin) and callable(pm.SimpleBatchPianoPIR.QueryFinish)
    assert pm.lib().pm_batchpir_client_max_sets(None, 96) == 0


def test_header_declares_them():
    text = (Path(__file__).resolve().parent.parent / "include" / "pacmann.h").read_text()
    flat = " ".join(text.split())
    assert "uint64_t pm_batchpir_client_max_sets(pm_batchpir* h, uint64_t n);" in flat
    assert ("int pm_batchpir_client_begin(pm_batchpir* h, const uint64_t* ids, uint64_t n, uint32_t* parts /* cap */, "
            "uint32_t* offsets /* cap x stride */, uint64_t stride, uint64_t cap, uint64_t* nq);") in flat
    assert ("int pm_batchpir_client_finish(pm_batchpir* h, const uint64_t* answers /* nq x DBEntrySize */, "
            "uint64_t nq, uint64_t* out /* n x DBEntrySize */, uint8_t* ok /* n, nullable */);") in flat
    assert "NO ABORT" in text   # the header says that begin cannot be undone


def test_null_handle_is_refused():
    import pacmann_amd as pm
    L = pm.lib()
    ids = np.zeros(4, dtype=np.uint64)
    parts = np.full(4, 7, dtype=np.uint32)
    offs = np.full((4, 8), 7, dtype=np.uint32)
    out = np.full((4, 2), 0xA5A5, dtype=np.uint64)
    nq = pm.u64(99)
    assert L.pm_ctx_mem_info(None, None, None) == PM_EINVAL   # another text first
    assert L.pm_batchpir_client_begin(None, ids.ctypes.data_as(pm.u64p), 4, parts.ctypes.data_as(pm.u32p),
                                      offs.ctypes.data_as(pm.u32p), 8, 4, C.byref(nq)) == PM_EINVAL
    assert L.pm_last_error().startswith(b"NULL argument")
    assert L.pm_ctx_mem_info(None, None, None) == PM_EINVAL
    assert L.pm_batchpir_client_finish(None, out.ctypes.data_as(pm.u64p), 1, out.ctypes.data_as(pm.u64p), None) == PM_EINVAL
    assert L.pm_last_error().startswith(b"NULL argument")
    assert nq.value == 99 and (parts == 7).all() and (offs == 7).all() and (out == 0xA5A5).all()


def test_wrapper_refuses_bad_answers():
    """Before the C call: a silent cast or reshape would hide the caller's mistake."""
    import pacmann_amd as pm
    p = pm.SimpleBatchPianoPIR.__new__(pm.SimpleBatchPianoPIR)
    p.h, p.E, p._owned = None, 4, False   # a NULL handle: a call that reached the library would say "NULL argument"
    with pytest.raises(TypeError, match="answers must be uint64"):
        p.QueryFinish(np.zeros((2, 4), dtype=np.int64))
    with pytest.raises(ValueError, match=r"answers must be \[nq, DBEntrySize\]"):
        p.QueryFinish(np.zeros(8, dtype=np.uint64))
    with pytest.raises(ValueError, match=r"answers must be \[nq, DBEntrySize\]"):
        p.QueryFinish(np.zeros((2, 5), dtype=np.uint64))
