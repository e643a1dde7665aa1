"""The streamed-preprocessing ABI (pm_batchpir_create_remote, pm_batchpir_prep_stream_*, pm_batchpir_prep_due,
pm_batchpir_server_rows) exists with the header's signatures, is bound in Python, and refuses NULL handles and bad
creation arguments with PM_EINVAL before any HIP call (no device needed)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
PM_EINVAL = -1   # include/pacmann.h

# name -> (result, parameter types) as include/pacmann.h declares them
DECLARED = {
    "pm_batchpir_create_remote": ("int", ["pm_ctx*", "uint64_t", "uint64_t", "uint64_t", "uint64_t", "uint64_t",
                                          "pm_batchpir**"]),
    "pm_batchpir_prep_stream_begin": ("int", ["pm_batchpir*"]),
    "pm_batchpir_prep_stream_rows": ("int", ["pm_batchpir*", "uint32_t", "uint32_t", "uint32_t", "const uint64_t*",
                                             "uint64_t"]),
    "pm_batchpir_prep_stream_end": ("int", ["pm_batchpir*"]),
    "pm_batchpir_prep_due": ("int", ["pm_batchpir*"]),
    "pm_batchpir_server_rows": ("int", ["pm_batchpir*", "uint32_t", "uint32_t", "uint32_t", "uint64_t*", "uint64_t",
                                        "uint64_t*"]),
}
CTYPES = {"int": C.c_int, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}


def header_signature(name):
    src = (ROOT / "include" / "pacmann.h").read_text()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    params = []
    for p in m.group(2).split(","):
        toks = p.replace("*", " * ").split()
        if len(toks) > 1 and re.fullmatch(r"[A-Za-z_]\w*", toks[-1]):   # the parameter's name
            toks = toks[:-1]
        params.append(" ".join(toks).replace(" *", "*"))
    return m.group(1), params


def test_header_declares_the_six_symbols():
    for name, (res, params) in DECLARED.items():
        got_res, got = header_signature(name)
        assert got_res == res, name
        assert got == params, (name, got)


def test_symbols_are_exported_and_bound():
    import pacmann_amd as pm
    L = pm.lib()
    for name, (res, params) in DECLARED.items():
        assert hasattr(L, name), name
        cres, cargs = pm.SIGNATURES[name]
        assert cres is CTYPES[res], name
        assert len(cargs) == len(params), name
        for a, p in zip(cargs, params):
            if p in CTYPES:
                assert a is CTYPES[p], (name, p)
            else:   # a pointer
                assert a in (pm.vp, pm.u64p) or a._type_ is pm.vp, (name, p)
    for meth in ("Remote", "PrepStreamBegin", "PrepStreamRows", "PrepStreamEnd", "ServerRows",
                 "StreamPreprocessingFrom"):
        assert callable(getattr(pm.SimpleBatchPianoPIR, meth)), meth
    assert isinstance(pm.SimpleBatchPianoPIR.prep_due, property)


def test_null_handles_are_refused():
    import pacmann_amd as pm
    L = pm.lib()
    rows = np.zeros((4, 8), dtype=np.uint64)
    n = C.c_uint64(77)
    calls = [
        lambda: L.pm_batchpir_prep_stream_begin(None),
        lambda: L.pm_batchpir_prep_stream_rows(None, 0, 0, 1, rows.ctypes.data_as(pm.u64p), 4),
        lambda: L.pm_batchpir_prep_stream_end(None),
        lambda: L.pm_batchpir_server_rows(None, 0, 0, 1, rows.ctypes.data_as(pm.u64p), 4, C.byref(n)),
    ]
    for i, call in enumerate(calls):
        assert L.pm_ctx_mem_info(None, None, None) == PM_EINVAL and L.pm_last_error() == b"ctx is NULL"   # another text first
        assert call() == PM_EINVAL, i
        assert L.pm_last_error() == b"NULL argument", (i, L.pm_last_error())
    assert n.value == 77 and not rows.any()
    assert L.pm_batchpir_prep_due(None) == 0


def test_create_remote_refuses_before_any_hip_call():
    import pacmann_amd as pm
    L = pm.lib()
    h = C.c_void_p(1)   # a non-NULL context that no check before the HIP calls may touch
    out = C.c_void_p()
    op = C.byref(out)
    cases = [
        (lambda: L.pm_batchpir_create_remote(None, 1000, 64, 8, 4, 1, op), b"ctx is NULL"),
        (lambda: L.pm_batchpir_create_remote(h, 0, 64, 8, 4, 1, op), b"DBSize must be > 0"),
        (lambda: L.pm_batchpir_create_remote(h, 1000, 7, 8, 4, 1, op), b"DBEntryByteNum must be >= 8"),
        (lambda: L.pm_batchpir_create_remote(h, 1000, 0, 8, 4, 1, op), b"DBEntryByteNum must be >= 8"),
        (lambda: L.pm_batchpir_create_remote(h, 1000, 64, 1, 4, 1, op), b"BatchSize must be >= 2"),
        (lambda: L.pm_batchpir_create_remote(h, 1000, 64, 0, 4, 1, op), b"BatchSize must be >= 2"),
        (lambda: L.pm_batchpir_create_remote(h, 1000, 64, 8, 4, 1, None), b"out is NULL"),
    ]
    for i, (call, want) in enumerate(cases):
        assert L.pm_ctx_mem_info(None, None, None) == PM_EINVAL and L.pm_last_error() == b"ctx is NULL"
        assert call() == PM_EINVAL, i
        assert L.pm_last_error() == want, (i, L.pm_last_error())
    assert out.value is None
