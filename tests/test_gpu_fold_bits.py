"""The bit-packed CS-512 fold (pmk::FOLD_ROT512Q) against the oracle, bit for bit.

A graph DB whose coordinates are f32 holding 0..255 and whose ids are below 2^20
has, beside the zero low halves that FOLD_ROT512P drops, a clear sign, three
exponent bits that copy a fourth, and twelve zero high id bits in every row.
The server finds that in its one pass over the rows (k_row_bits_or) and builds an
image of 12-bit coordinate and 20-bit id fields, whole quads of four fields per
32-B slice; k_prep_fold_rot<512> folds the fewer slices as before and its
epilogue expands the fields into whole parity words.  "host_fold_rot512q" counts
those launches and adds up the slices they folded, which tells the forms apart:
both kinds of field, 12-bit coordinates alone, 20-bit ids alone.

Shapes: partitions of 16,600 rows (ChunkSize 512, a partial last chunk: rows
past N in the image), the smallest that reach the rotated fold.
  dim 64,  m 8   4 partitions    4 slices (the packed image has 5)
  dim 64,  m 12  6 partitions    4 slices; E = 38 words, so two words past E & ~3
  dim 64,  m 32  16 partitions   6 slices (8)
  dim 128, m 32  16 partitions   9 slices (12): SIFT1M's rows
A DB whose last partition is one row short of the others is among them.

One coordinate or id of the last row decides the form of the dim 128 shape:
  65536.0  exponent 143 = 0b10001111: bits 6..3 differ, low half zero   20-bit ids alone, 11 slices
  an id of 2^20                                                          12-bit coordinates alone, 11 slices
  1 / 3    a non-zero low half                                           the plain image, rot512
  0.5 and 256.0  exponents 126 = 0b01111110 and 135 = 0b10000111: bits 6..3 are all
           ones, or all zero, the sign is clear and the low half zero.  They are no
           bytes, but they pass the reduction as 1.0 and 128.0 do and their fields
           expand exactly: the 9-slice form is the right one for such a DB, and its
           state must equal the oracle's.
"""
import numpy as np
import pytest

from tests.test_gpu_fold_forms import assert_state
from tests.test_gpu_parity import SEED

pytestmark = pytest.mark.gpu

PS = 16600
FORMS = ("rot512q", "rot512p", "rot512", "rot1024", "other")
# dim, m, rows, entry words, slices of the bit-packed image
SMALL = (64, 8, 4 * PS, 36, 4)
SHORT = (64, 8, 4 * PS - 1, 36, 4)      # the last partition one row short
ODD_E = (64, 12, 6 * PS, 38, 4)
WIDE_M = (64, 32, 16 * PS, 48, 6)
SIFT = (128, 32, 16 * PS, 80, 9)


@pytest.fixture
def fold_pack():
    """fold_pack(level): 2 "fold_pack" and "fold_bits" on, 1 "fold_bits" off, 0 "fold_pack" off."""
    import pacmann_amd as pm

    def level(v):
        pm.set_option("fold_pack", int(v > 0))
        pm.set_option("fold_bits", int(v > 1))
    try:
        yield level
    finally:
        pm.set_option("fold_pack", -1)
        pm.set_option("fold_bits", -1)


_data, _oracle = {}, {}


def data(shape, spoil=None):
    """Byte-valued vectors and a random graph; spoil = ("v", x): one coordinate of the DB's last
    row becomes x; ("id", x): one neighbour id of that row."""
    dim, m, N = shape[:3]
    if (shape, spoil) not in _data:
        rng = np.random.default_rng(N + dim + m)
        v = rng.integers(0, 256, size=(N, dim)).astype(np.float32)
        v[0, :2] = (0.0, 1.0)
        g = rng.integers(0, N, size=(N, m)).astype(np.uint32)
        if spoil is not None and spoil[0] == "v":
            v[N - 1, dim - 3] = spoil[1]
        elif spoil is not None:
            g[N - 1, m - 2] = spoil[1]
        _data[shape, spoil] = (v, g)
    return _data[shape, spoil]


def oracle_states(oracle, shape, spoil, pir_seed, epochs=1):
    key = (shape, spoil, pir_seed, epochs)
    if key not in _oracle:
        v, g = data(shape, spoil)
        o = oracle.Graph(v, g, pir_seed=pir_seed, search_seed=1)
        o.Preprocess()
        for _ in range(epochs - 1):
            o.pir().Preprocessing()
        _oracle[key] = [o.pir().sub(p).export_state() for p in range(shape[1] // 2)]
    return _oracle[key]


def counts(c):
    return {k: c.timing_get("host_fold_" + k)[0] for k in FORMS}


def only(form, n=1):
    return dict(dict.fromkeys(FORMS, 0), **{form: n})


def slices_folded(c):
    return c.timing_get("host_fold_rot512q")[1]


def assert_states(pir, want, E, what):
    for p in range(len(want)):
        assert pir.SubConfig(p)["ChunkSize"] == 512
        assert_state(pir.export_state(p), want[p], E, f"{what} partition {p}")


@pytest.mark.parametrize("shape", [SMALL, SHORT, ODD_E, WIDE_M, SIFT], ids=["d64m8", "short", "d64m12", "d64m32", "d128m32"])
def test_bit_packed_one_client(oracle, fold_pack, shape):
    """One client's Preprocessing(): one bit-packed launch of the expected slices, the whole
    exported state equal to the oracle's, then a few private fetches."""
    import pacmann_amd as pm
    fold_pack(2)
    dim, m, N, E, nsl = shape
    ctx = pm.Context(0)
    v, g = data(shape)
    base = pm.PIRGraphInfo(v, g, pir_seed=SEED, search_seed=5, ctx=ctx)
    ctx.timing_reset()
    base.Preprocess()
    assert counts(ctx) == only("rot512q") and slices_folded(ctx) == nsl
    pir = base.PIR
    last = pir.SubConfig(m // 2 - 1)
    assert last["DBSize"] % 512 and last["SetSize"] * 512 > last["DBSize"]   # padded rows in the image
    assert_states(pir, oracle_states(oracle, shape, None, SEED), E, "epoch 0")
    if shape in (SMALL, SHORT):
        o = oracle.Graph(v, g, pir_seed=SEED, search_seed=5)
        o.Preprocess()
        q = np.random.default_rng(N + 1).integers(0, N, size=256, dtype=np.uint64)
        q[:2] = (N - 1, 0)
        got, _ = pir.Query(q)
        want, _ = o.pir().Query(q)
        assert np.array_equal(got, want)


SEEDS = [(SEED, 5), (41, 6), (42, 7)]


@pytest.mark.parametrize("shape", [SMALL, ODD_E, SIFT], ids=["d64m8", "d64m12", "d128m32"])
def test_bit_packed_three_clients_one_launch(oracle, fold_pack, shape):
    """Three sessions re-preprocessed as one launch set: one bit-packed fold over virtual hint
    groups that span two clients.  The dim 128 shape has every kind of slice: coordinates alone,
    coordinates beside ids, ids alone."""
    import pacmann_amd as pm
    fold_pack(2)
    dim, m, N, E, nsl = shape
    ctx = pm.Context(0)
    v, g = data(shape)
    base = pm.PIRGraphInfo(v, g, pir_seed=SEEDS[0][0], search_seed=SEEDS[0][1], ctx=ctx)
    base.Preprocess()
    sess = [base] + [base.Session(p, s, pm.Context(0)) for p, s in SEEDS[1:]]
    for x in sess[1:]:
        x.Preprocess()
    pirs = [x.PIR for x in sess]
    grp = pm.BatchPIRGroup(pirs)
    ctx.timing_reset()
    ctx.timing(1)
    grp.Preprocessing()
    ctx.sync()
    ctx.timing(False)
    assert counts(ctx) == only("rot512q") and slices_folded(ctx) == nsl and ctx.timing_get("prep_fold")[0] == 1
    for pir, (ps, _) in zip(pirs, SEEDS):
        assert pir.stats()["PrepCount"] == 2
        assert_states(pir, oracle_states(oracle, shape, None, ps, epochs=2), E, f"client seed {ps}")


@pytest.mark.parametrize("spoil,form,nsl", [
    pytest.param(("v", 65536.0), "rot512q", 11, id="65536"),
    pytest.param(("v", 256.0), "rot512q", 9, id="256"),
    pytest.param(("v", 0.5), "rot512q", 9, id="half"),
    pytest.param(("id", 1 << 20), "rot512q", 11, id="id"),
    pytest.param(("v", 1.0 / 3.0), "rot512", 0, id="third"),
])
def test_one_word_decides(oracle, fold_pack, spoil, form, nsl):
    """One word of the last row of the last partition decides the form (module docstring)."""
    import pacmann_amd as pm
    fold_pack(2)
    dim, m, N, E, _ = SIFT
    ctx = pm.Context(0)
    v, g = data(SIFT, spoil)
    base = pm.PIRGraphInfo(v, g, pir_seed=SEED, search_seed=5, ctx=ctx)
    ctx.timing_reset()
    base.Preprocess()
    assert counts(ctx) == only(form) and slices_folded(ctx) == nsl
    assert_states(base.PIR, oracle_states(oracle, SIFT, spoil, SEED), E, str(spoil))


def test_small_shape_lesser_forms(oracle, fold_pack):
    """dim 64, m 8: 20-bit ids alone or 12-bit coordinates alone take 5 slices, no fewer than the
    packed image's, so such a DB keeps the packed image."""
    import pacmann_amd as pm
    fold_pack(2)
    for spoil in (("v", 65536.0), ("id", 1 << 20)):
        ctx = pm.Context(0)
        v, g = data(SMALL, spoil)
        base = pm.PIRGraphInfo(v, g, pir_seed=SEED, search_seed=5, ctx=ctx)
        ctx.timing_reset()
        base.Preprocess()
        assert counts(ctx) == only("rot512p")
        assert_states(base.PIR, oracle_states(oracle, SMALL, spoil, SEED), SMALL[3], str(spoil))


@pytest.mark.parametrize("opt,form", [(2, "rot512q"), (1, "rot512p"), (0, "rot512")])
def test_option_levels_and_sessions(oracle, fold_pack, opt, form):
    """Both options on / "fold_bits" off / "fold_pack" off when the server is created: bit-packed,
    packed (the launches of the build before this form), plain.  A session shares its base's image and form whatever the
    option says later, and every form gives the same state."""
    import pacmann_amd as pm
    fold_pack(opt)
    v, g = data(SMALL)
    base = pm.PIRGraphInfo(v, g, pir_seed=SEED, search_seed=5, ctx=pm.Context(0))
    base.ctx.timing_reset()
    base.Preprocess()
    assert counts(base.ctx) == only(form)
    fold_pack(2 if opt == 0 else 0)
    s = base.Session(41, 6, pm.Context(0))
    s.ctx.timing_reset()
    s.Preprocess()
    assert counts(s.ctx) == only(form)
    assert_states(base.PIR, oracle_states(oracle, SMALL, None, SEED), SMALL[3], "base")
    assert_states(s.PIR, oracle_states(oracle, SMALL, None, 41), SMALL[3], "session")
