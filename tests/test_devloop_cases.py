"""The device-loop round cases (tests/devloop_cases.py) on the oracle alone: every case reaches the branches it
is meant for, by the oracle's own trace counts, and its shape is on the intended side of the gate.  No GPU."""
import pytest

from tests import devloop_cases as D


@pytest.mark.parametrize("name", [c.name for c in D.CASES])
def test_case_reaches_its_branches(oracle, name):
    case = D.BY_NAME[name]
    got = D.trace_sum(D.oracle_run(oracle, case))
    print(name, got)
    for key, want in case.expect.items():
        if want == D.SOME:
            assert 0 < got["succ"] < got["total"], (got["succ"], got["total"])
        elif isinstance(want, tuple):
            assert want[0] == ">" and got[key] > want[1], (key, got[key], want)
        else:
            assert got[key] == want, (key, got[key], want)


@pytest.mark.parametrize("name", [c.name for c in D.CASES])
def test_case_gate(name):
    case = D.BY_NAME[name]
    assert D.gate(case) == case.gate
    assert 2 <= case.S <= 5 and 2 <= case.q <= 3 and (case.dim + case.m) % 2 == 0
    if not case.gate and "succ" in case.expect:   # whole lists exactly where the entry is a multiple of 4 words
        assert ((case.dim + case.m) // 2 % 4 == 0) == (case.expect["succ"] == D.SOME)


def test_decode_forms():
    """Both scalar reasons (m / 4 no power of two; odd E) and the vector decode's 1, 2, 4, 8 and 16 chunks."""
    dev = [c for c in D.CASES if not c.gate]
    scalar = {c.name for c in dev if not D.vec16(c)}
    assert scalar == {"scalar-m24", "scalar-m24-whole", "scalar-dim102", "scalar-dim102-m26"}
    # every decode form compares at least one entry that equals the true list and one that does not
    for name in scalar - {"scalar-m24", "scalar-dim102"} | {"vec-m4", "vec-m8", "vec-m16", "vec-m64", "n256-random"}:
        assert D.BY_NAME[name].expect["succ"] == D.SOME, name
    assert (D.BY_NAME["scalar-dim102"].dim + 32) // 2 % 2 == 1 and D.BY_NAME["scalar-m24"].dim % 4 == 0
    assert {c.m // 4 for c in dev if D.vec16(c)} == {1, 2, 4, 8, 16}
    assert {c.parallel for c in dev} >= {1, 2, 3, 8}
    assert {c.parallel * c.m for c in dev} >= {256, 96, 32}


def test_generators():
    import numpy as np
    from tests import datagen
    n, m, w = 512, 8, 8
    g = datagen.windowed_graph(n, m, w, seed=1)
    d = (g.astype(np.int64) - np.arange(n)[:, None] + n // 2) % n - n // 2
    assert g.dtype == np.uint32 and g.shape == (n, m) and (np.abs(d) <= w).all() and (d != 0).all()
    assert np.array_equal(g, datagen.windowed_graph(n, m, w, seed=1))
    lone = datagen.lone_id_lists(g, 8, seed=1)
    assert np.array_equal(g, datagen.windowed_graph(n, m, w, seed=1))   # a copy: g is unchanged
    assert ((lone[4::8] != 0).sum(1) == 1).all() and np.array_equal(np.delete(lone, np.s_[4::8], 0), np.delete(g, np.s_[4::8], 0))
    s = datagen.sparse_graph(n, m, 0.25, seed=1)
    kept = s.any(1)
    assert 0.15 < kept.mean() < 0.35 and np.array_equal(s[kept], datagen.random_graph(n, m, seed=1)[kept])
    assert not datagen.sparse_graph(n, m, 0.0, seed=1).any()
    z = datagen.vertex0_graph(n, m, seed=1)
    assert (z[1::2] == 0).any(1).all() and ((z[4::8] != 0).sum(1) == 1).all() and z[0].any()
    v, protos = datagen.tied_vectors(n, 16, 64, seed=1)
    assert v.dtype == np.float32 and protos.shape == (64, 16) and (v == np.rint(v)).all()
    assert all((v == p).all(1).sum() == n // 64 for p in protos)


def test_every_branch_has_a_case():
    assert len(D.BRANCHES) == 13
    for branch, names in D.BRANCHES.items():
        assert names and all(n in D.BY_NAME for n in names), branch
    assert {n for names in D.BRANCHES.values() for n in names} | {"step1"} == set(D.BY_NAME)
