"""The packed CS-512 fold (pmk::FOLD_ROT512P) against the oracle.

A graph DB whose f32 coordinates are all integer-valued (SIFT's bytes) has zero
low halves in every coordinate word, so in every parity.  The server detects
that once, builds a fold image without those halves, and k_prep_fold_rot<512>
folds dim / 16 packed coordinate slices plus the neighbour-id slices instead of
(dim + m) / 8 whole ones.  "host_fold_rot512p" counts those folds,
"host_fold_rot512" the ones over a plain image.

The shapes are test_gpu_fold_forms.py's smallest CS-512 ones, 80,000 and 66,400
rows in four partitions, as graph DBs of dim 32, m 8 (E = 20 words: two packed
slices and one id slice in place of five).  Partitions of 20,000 / 16,600 rows
end mid-chunk, so zero-padded rows pass through the packed image.  A graph's
batch PIR is always created with FailureProbLog2 8, so the 66,400-row shape has
7,328 hints per partition here, not the 4,768 that the raw F = 1 engine of
test_gpu_fold_forms.py folds in per-client groups: both shapes take virtual hint
groups, and with three clients in one launch set a group spans two clients."""
import numpy as np
import pytest

from tests.test_gpu_fold_forms import assert_state
from tests.test_gpu_parity import SEED

pytestmark = pytest.mark.gpu

DIM, M, E, P, CS = 32, 8, 20, 4, 512
SHAPES = [pytest.param(80000, 40, 8064, id="80000"), pytest.param(66400, 36, 7328, id="66400")]
SEEDS = [(SEED, 5), (41, 6), (42, 7)]


@pytest.fixture
def fold_pack():
    import pacmann_amd as pm
    try:
        yield lambda v: pm.set_option("fold_pack", v)
    finally:
        pm.set_option("fold_pack", -1)


_data, _oracle = {}, {}


def data(N, spoil=None):
    """Integer-valued vectors and a random graph; spoil: the value of one coordinate of the
    DB's last row (the last chunk of the last partition)."""
    if (N, spoil) not in _data:
        rng = np.random.default_rng(N)
        v = rng.integers(0, 256, size=(N, DIM)).astype(np.float32)
        g = rng.integers(0, N, size=(N, M)).astype(np.uint32)
        if spoil is not None:
            v[N - 1, DIM - 3] = spoil
        _data[N, spoil] = (v, g)
    return _data[N, spoil]


def oracle_states(oracle, N, spoil, pir_seed, epochs=1):
    """The oracle client's partitions' states after `epochs` preprocessings, computed once."""
    key = (N, spoil, pir_seed, epochs)
    if key not in _oracle:
        v, g = data(N, spoil)
        o = oracle.Graph(v, g, pir_seed=pir_seed, search_seed=1)
        o.Preprocess()
        for _ in range(epochs - 1):
            o.pir().Preprocessing()
        _oracle[key] = [o.pir().sub(p).export_state() for p in range(P)]
    return _oracle[key]


def counts(c):
    return {k: c.timing_get("host_fold_" + k)[0] for k in ("rot512p", "rot512", "rot1024", "other")}


def only(form, n=1):
    return dict({"rot512p": 0, "rot512": 0, "rot1024": 0, "other": 0}, **{form: n})


def check_geometry(pir, N, SS, H):
    for p in range(P):
        c = pir.SubConfig(p)
        assert (c["DBSize"], c["ChunkSize"], c["SetSize"]) == (N // P, CS, SS)
        assert c["PrimaryHintNum"] + c["SetSize"] * c["MaxQueryPerChunk"] == H
        assert c["DBSize"] % CS and c["SetSize"] * CS > c["DBSize"]   # the last chunk is partial: padded rows


def assert_states(pir, want, what):
    for p in range(P):
        assert_state(pir.export_state(p), want[p], E, f"{what} partition {p}")


@pytest.mark.parametrize("N,SS,H", SHAPES)
def test_packed_one_client(oracle, N, SS, H):
    """One client: the state after Preprocessing() and after a query sequence
    that crosses a re-preprocessing, every fold of it a packed one."""
    import pacmann_amd as pm
    ctx = pm.Context(0)
    v, g = data(N)
    base = pm.PIRGraphInfo(v, g, pir_seed=SEED, search_seed=5, ctx=ctx)
    ctx.timing_reset()
    base.Preprocess()
    assert counts(ctx) == only("rot512p")
    pir = base.PIR
    check_geometry(pir, N, SS, H)
    assert_states(pir, oracle_states(oracle, N, None, SEED), "epoch 0")
    o = oracle.Graph(v, g, pir_seed=SEED, search_seed=5)
    o.Preprocess()
    rng = np.random.default_rng(N + 1)
    n, maxq = 1024, pir.SubConfig(0)["MaxQueryNum"]
    for b in range(int(maxq // (n // P)) + 3):
        q = rng.integers(0, N, size=n, dtype=np.uint64)
        got, _ = pir.Query(q)
        want, _ = o.pir().Query(q)
        assert np.array_equal(got, want), b
    assert pir.stats()["PrepCount"] == o.pir().stats()["PrepCount"] == 2
    for p in range(P):
        assert_state(pir.export_state(p), o.pir().sub(p).export_state(), E, f"after the sequence, partition {p}")
    c = counts(ctx)
    assert c["rot512p"] >= 2 and c["rot512"] == c["rot1024"] == c["other"] == 0, c


@pytest.mark.parametrize("N,SS,H", SHAPES)
def test_packed_three_clients_one_launch(oracle, N, SS, H):
    """Three sessions re-preprocessed as one launch set: one packed fold whose
    virtual hint groups of 5,120 span two clients (H is not a multiple)."""
    import pacmann_amd as pm
    ctx = pm.Context(0)
    v, g = data(N)
    base = pm.PIRGraphInfo(v, g, pir_seed=SEEDS[0][0], search_seed=SEEDS[0][1], ctx=ctx)
    base.Preprocess()
    sess = [base] + [base.Session(p, s, pm.Context(0)) for p, s in SEEDS[1:]]
    for x in sess[1:]:
        x.Preprocess()
    assert H % 5120 and 5120 < H
    pirs = [x.PIR for x in sess]
    grp = pm.BatchPIRGroup(pirs)
    ctx.timing_reset()
    ctx.timing(1)
    grp.Preprocessing()     # epoch 1, on the first client's context
    ctx.sync()
    ctx.timing(False)
    assert counts(ctx) == only("rot512p") and ctx.timing_get("prep_fold")[0] == 1
    for pir, (ps, _) in zip(pirs, SEEDS):
        assert pir.stats()["PrepCount"] == 2
        assert_states(pir, oracle_states(oracle, N, None, ps, epochs=2), f"client seed {ps}")


@pytest.mark.parametrize("value,form", [
    # 0.5 = 0x3f000000: not an integer, but its low half is zero, so nothing the packed image drops
    pytest.param(0.5, "rot512p", id="half"),
    # 1/3 = 0x3eaaaaab: the detector must refuse
    pytest.param(1.0 / 3.0, "rot512", id="third"),
])
@pytest.mark.parametrize("N,SS,H", SHAPES)
def test_one_coordinate_decides(oracle, N, SS, H, value, form):
    """One coordinate of the last row of the last partition (its last, partial
    chunk): a non-zero low half there alone turns the packed image off."""
    import pacmann_amd as pm
    ctx = pm.Context(0)
    v, g = data(N, value)
    bits = int(v[N - 1, DIM - 3].view(np.uint32))
    assert (bits & 0xffff == 0) == (form == "rot512p")
    assert not (np.delete(v.view(np.uint32).ravel(), (N - 1) * DIM + DIM - 3) & 0xffff).any()
    base = pm.PIRGraphInfo(v, g, pir_seed=SEED, search_seed=5, ctx=ctx)
    ctx.timing_reset()
    base.Preprocess()
    assert counts(ctx) == only(form)
    check_geometry(base.PIR, N, SS, H)
    assert_states(base.PIR, oracle_states(oracle, N, value, SEED), f"{value}")


@pytest.mark.parametrize("opt,form", [(1, "rot512p"), (0, "rot512")])
def test_session_shares_image_and_decision(oracle, fold_pack, opt, form):
    """A Session shares its base's image, so its form, whatever "fold_pack" says
    when the session is created."""
    import pacmann_amd as pm
    N = 80000
    v, g = data(N)
    fold_pack(opt)
    base = pm.PIRGraphInfo(v, g, pir_seed=SEED, search_seed=5, ctx=pm.Context(0))
    base.ctx.timing_reset()
    base.Preprocess()
    assert counts(base.ctx) == only(form)
    fold_pack(1 - opt)
    s = base.Session(41, 6, pm.Context(0))
    s.ctx.timing_reset()
    s.Preprocess()
    assert counts(s.ctx) == only(form)
    assert_states(s.PIR, oracle_states(oracle, N, None, 41), "session")
    if opt == 0:   # the plain image of an integer-valued DB: the same state as the packed one
        assert_states(base.PIR, oracle_states(oracle, N, None, SEED), "base")


def test_raw_engine_never_packs(ctx, oracle):
    """The same rows given to a bare batch PIR engine: no entry layout, no packed image."""
    import pacmann_amd as pm
    N = 80000
    v, g = data(N)
    raw = np.concatenate([v.view(np.uint32), g], axis=1).reshape(-1).view(np.uint64)
    pir = pm.SimpleBatchPianoPIR(N, E * 8, M, raw, 8, seed=SEED, ctx=ctx)
    ctx.timing_reset()
    pir.Preprocessing()
    assert counts(ctx) == only("rot512")
    assert_states(pir, oracle_states(oracle, N, None, SEED), "raw engine")
