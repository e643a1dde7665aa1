"""The C-ABI library loads and exports every symbol include/pacmann.h declares
(no compute calls: this runs without a GPU)."""
import ctypes as C
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def declared_symbols():
    src = (ROOT / "include" / "pacmann.h").read_text()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pm_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_api():
    syms = declared_symbols()
    for s in ("pm_ctx_create", "pm_prf_batch", "pm_pir_server_answer", "pm_batchpir_query", "pm_batchpir_step_spec",
              "pm_search_knn", "pm_l2_batch", "pm_ip_bench"):
        assert s in syms


def test_library_exports_every_symbol():
    import pacmann_amd as pm
    L = pm.lib()   # raises if the .so is missing: no fallback
    missing = [s for s in declared_symbols() if not hasattr(L, s)]
    assert not missing, missing


def test_python_binding_covers_header():
    import pacmann_amd as pm
    assert set(declared_symbols()) == set(pm.SIGNATURES)


def test_host_key_schedule_matches_oracle(oracle):
    """pm_expand_key is host code (no device needed)."""
    import numpy as np
    import pacmann_amd as pm
    rng = np.random.default_rng(0)
    for _ in range(10):
        k = rng.bytes(16)
        assert np.array_equal(pm.expand_key(k), oracle.expand_key(k))


def test_last_error_crosses_files():
    """One argument-checked entry point of every host file (csrc/pm_*.cpp, one
    per layer): each fails with PM_EINVAL before any HIP call, and
    pm_last_error, which lives in pm_ctx.cpp, returns that call's text: the
    error text is one per thread, not one per file."""
    import pacmann_amd as pm
    L = pm.lib()
    PM_EINVAL = -1   # include/pacmann.h
    out = C.c_void_p()
    cases = [
        ("context", lambda: L.pm_ctx_create(0, None), b"out is NULL"),
        ("engine", lambda: L.pm_pir_create(None, 16, 8, None, 8, 1, None), b"out is NULL"),
        ("search", lambda: L.pm_graph_create(None, 1, 1, 1, None, None, 0, 0, 1, 1, C.byref(out)),
         b"NULL argument"),
        ("group", lambda: L.pm_batchpir_group_create(None, 0, None), b"NULL argument"),
        ("device loop", lambda: L.pm_search_loop_batched(None, 0, None, 0, 1, 1, 1, 1, 1, None, None, None, None),
         b"NULL argument"),
        ("rccl", lambda: L.pm_rccl_create(0, 1, 0, None, 1, C.byref(out)), b"bad argument"),
        ("graph build", lambda: L.pm_knn(None, None, 1, 1, None, 0, 1, None, None), b"NULL argument"),
    ]
    for layer, call, want in cases:
        # another text first (set in pm_ctx.cpp), so that an equal text of the case before cannot pass for this one
        assert L.pm_ctx_mem_info(None, None, None) == PM_EINVAL
        assert L.pm_last_error() == b"ctx is NULL"
        assert call() == PM_EINVAL, layer
        assert L.pm_last_error() == want, layer


def test_step_spec_argument_checks():
    """pm_batchpir_step_spec checks its arguments before it touches the handle or the device; the texts of its
    other refusals (a context without the record, a last step that was not k_step's) are pinned where a step can
    run: tests/test_gpu_step_spec.py::test_step_spec_errors."""
    import pacmann_amd as pm
    L = pm.lib()
    out, n = (C.c_uint32 * 4)(), C.c_uint64(0)
    handle = C.c_void_p(1)   # never dereferenced: a NULL argument is refused first
    for args in ((None, out, 4, C.byref(n)), (handle, None, 4, C.byref(n)), (handle, out, 4, None),
                 (None, None, 0, C.byref(n)), (handle, None, 0, None)):
        assert L.pm_ctx_mem_info(None, None, None) == -1 and L.pm_last_error() == b"ctx is NULL"
        assert L.pm_batchpir_step_spec(*args) == -1
        assert L.pm_last_error() == b"NULL argument"
    assert pm.step_spec_fields(0x80000000 | 1 | 8 | 16 | 32 | (1 << 8)) == dict(
        gmode=1, helped=True, help_ok=True, kept=True, redo=False, mode=1, written=True)
    assert pm.step_spec_fields(0x80000000 | 7 | 64 | (3 << 8)) == dict(
        gmode=7, helped=False, help_ok=False, kept=False, redo=True, mode=3, written=True)


def test_build_lists_cover_csrc():
    """Every source and header under csrc/ is in the build lists, so that
    needs_build() sees a change to any of them and no file is left unlinked."""
    from pacmann_amd import build
    csrc = ROOT / "pacmann_amd" / "csrc"
    sources = sorted(p for p in csrc.iterdir() if p.suffix in (".hip", ".cpp"))
    headers = sorted(csrc.glob("*.h"))
    assert sources and headers
    assert [p for p in sources if p not in build.SOURCES] == []
    assert [p for p in headers if p not in build.HEADERS] == []


def test_no_gpu_raises_loudly():
    """Without a HIP device the product must fail, never fall back to CPU."""
    import pacmann_amd as pm
    import pytest
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        pm.Context(0)


def test_oracle_not_used_by_product():
    """The product never imports, links or loads the oracle (test infrastructure)."""
    for p in (ROOT / "pacmann_amd").rglob("*"):
        if p.suffix in (".py", ".cpp", ".hip", ".h"):
            t = p.read_text()
            assert not re.search(r"import\s+oracle|from\s+oracle|liboracle|pm_oracle\.h", t), p
