"""Every form of the maintenance hint fold against the oracle.

pmk::fold_form (pm_kernels.hip) picks the fold of a preprocessing from the
partitions' ChunkSize range, the entry words E and whether the engine was
created with a fold image:

  rot512 / rot1024  k_prep_fold_rot<512 / 1024>   one CS of 512 / 1,024, image
  pipe              k_prep_fold_pipe<4,1> <4,2,3> <2,2,3>   one CS of 512 /
                    1,024 (no image: pm_set_option("fold_rot", 0), an image
                    that does not fit, a client of a server without one) /
                    2,048
  blk               k_prep_fold_blk<8 / 4 / 2>    every other even E >= 4,
                    mixed ChunkSizes in one batch PIR included
  gather            k_prep_fold<1 / 2>            odd E, E < 4

Each case builds the product and the oracle on one seeded random DB, runs
Preprocessing() on both and requires the whole exported client state to be
equal bit for bit (XORs of 64-bit words: the tolerance is zero,
Client.Preprocessing pir.go:267-352).  Each case also asserts the geometry it
relies on (ChunkSize, SetSize, hint count, from Config() and the exported tag
arrays) and, from the "host_fold_*" counters, that exactly the expected form
ran: a change to the parameterisation or to the selection cannot silently move
a case onto a sibling kernel.
"""
import numpy as np
import pytest

from tests.test_gpu_parity import SEED, STATE_KEYS, rand_db

pytestmark = pytest.mark.gpu

FORMS = ("rot512", "rot1024", "pipe", "blk", "gather")


@pytest.fixture
def fold_rot():
    """Sets pm_set_option("fold_rot", v); the environment's choice is restored afterwards."""
    import pacmann_amd as pm
    try:
        yield lambda v: pm.set_option("fold_rot", v)
    finally:
        pm.set_option("fold_rot", -1)


def fold_counts(c):
    return {k: c.timing_get("host_fold_" + k)[0] for k in FORMS + ("other",)}


def assert_only(c, form, n=1):
    """Exactly `form` was launched, n times; "other" = every launch that is not a rotated one."""
    want = dict.fromkeys(FORMS + ("other",), 0)
    want[form] = n
    if not form.startswith("rot"):
        want["other"] = n
    got = fold_counts(c)
    assert got == want, (got, want)


def assert_state(a, b, E, what=""):
    """Bit-equal state; a parity mismatch is reported as (hint, word) pairs."""
    for k in STATE_KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (what, k)
        if not np.array_equal(x, y):
            d = np.where(x != y)[0]
            where = [(int(i // E), int(i % E)) for i in d[:8]] if k.endswith(("parity", "val")) else d[:8].tolist()
            raise AssertionError(f"{what} {k}: {len(d)} of {x.size} differ, first (hint, word) {where}, "
                                 f"last {int(d[-1] // E) if k.endswith(('parity', 'val')) else int(d[-1])}")


def hints(state):
    return len(state["primary_tag"]) + len(state["backup_tag"])


_oracle_state = {}


def oracle_pir_state(oracle, N, E, F):
    """The oracle's Config and state after Preprocessing(), computed once per shape."""
    key = (N, E, F)
    if key not in _oracle_state:
        o = oracle.PianoPIR(N, E * 8, rand_db(N, E, seed=N + E), F, seed=SEED)
        o.Preprocessing()
        _oracle_state[key] = (o.Config(), o.export_state())
    return _oracle_state[key]


# (rows, E words, F) -> ChunkSize, SetSize, hints, the form with "fold_rot" 0 and with 1
# (None: the option does not bear on the shape, run once at the environment's choice)
SINGLE = [
    # one slice; three pipelined hint groups, the last short; chunk 36 partial, 37-39 past N
    ((18750, 4, 40), (512, 40, 19008), "pipe", "rot512"),
    # 20 slices = five 128-B line groups
    ((62500, 80, 8), (512, 124, 12512), "pipe", "rot512"),
    # E % 4 == 2: parity words 4-5 zero, one image slice
    ((20000, 6, 8), (512, 40, 8064), "pipe", "rot512"),
    # two slices and tail words
    ((20000, 10, 8), (512, 40, 8064), "pipe", "rot512"),
    # fewer hints than a rotated group's 5,120 lane slots: the per-client groups (ngc != 0)
    ((16600, 4, 1), (512, 36, 4768), "pipe", "rot512"),
    # two slices; three groups with hb rounded up to 8 and a short last one; chunk 68 partial, 69-71 past N
    ((70000, 8, 8), (1024, 72, 15808), "pipe", "rot1024"),
    # tail words at CS 1,024
    ((100000, 6, 8), (1024, 100, 18368), "pipe", "rot1024"),
    # k_prep_fold_pipe<2,2,3>: two slices of an eight-slice line group (no image at CS 2,048)
    ((270000, 6, 8), (2048, 132, 34400), "pipe", None),
    # the only k_prep_fold_blk<2> shape (1,048,576 < rows <= 4,194,304)
    ((1100000, 4, 8), (4096, 272, 72192), "blk", None),
    # k_prep_fold_blk<8> for words 0-7, then <4> for words 8-11
    ((5000, 12, 8), (256, 20, 3712), "blk", None),
    # the unblocked gather: odd E (k_prep_fold<1>, tail word zero) and E < 4 (zero parities)
    ((3000, 5, 8), (128, 24, 2240), "gather", None),
    ((2000, 2, 8), (128, 16, 1920), "gather", None),
]
SINGLE_CASES = [pytest.param(*shape, geom, opt, form, id=f"{shape[0]}x{shape[1]}-F{shape[2]}-opt{opt}-{form}")
                for shape, geom, f0, f1 in SINGLE
                for opt, form in (((0, f0), (1, f1)) if f1 else ((-1, f0),))]


@pytest.mark.parametrize("N,E,F,geom,opt,form", SINGLE_CASES)
def test_fold_form_state(ctx, oracle, fold_rot, N, E, F, geom, opt, form):
    import pacmann_amd as pm
    fold_rot(opt)
    g = pm.PianoPIR(N, E * 8, rand_db(N, E, seed=N + E), F, seed=SEED, ctx=ctx)
    ocfg, ostate = oracle_pir_state(oracle, N, E, F)
    cfg = g.Config()
    assert cfg == ocfg
    assert (cfg["ChunkSize"], cfg["SetSize"]) == geom[:2]
    assert cfg["PrimaryHintNum"] + cfg["SetSize"] * cfg["MaxQueryPerChunk"] == geom[2]
    ctx.timing_reset()
    g.Preprocessing()
    assert_only(ctx, form)
    state = g.export_state()
    assert hints(state) == geom[2]   # the exported tag arrays carry the hint count the kernels grouped
    assert_state(state, ostate, E)
    if E % 4:   # xorSlices (aes_amd64.s:133-157) leaves the words past E & ~3 zero
        assert not state["primary_parity"].reshape(-1, E)[:, E & ~3:].any()


def batch_geometry(g, want):
    """[(ChunkSize, SetSize, hints)] of every partition, asserted against `want`."""
    got = []
    for p in range(g.Config()["PartitionNum"]):
        c = g.SubConfig(p)
        got.append((c["ChunkSize"], c["SetSize"], c["PrimaryHintNum"] + c["SetSize"] * c["MaxQueryPerChunk"]))
    assert got == want, got


def test_mixed_chunk_size_batch(ctx, oracle):
    """Partitions of 16,513 rows (CS 512) and 16,510 rows (CS 256) in one
    batch PIR: the double-buffered fold with LDS sized by the larger ChunkSize,
    and every online kernel (PRF tables, hint search, answer, refresh) over two
    geometries in one launch, through the batch layer's re-preprocessing."""
    import pacmann_amd as pm
    N, E, B, n = 66049, 8, 8, 96
    db = rand_db(N, E, N + E)
    g = pm.SimpleBatchPianoPIR(N, E * 8, B, db, 8, seed=SEED, ctx=ctx)
    o = oracle.SimpleBatchPianoPIR(N, E * 8, B, db, 8, seed=SEED)
    assert g.Config()["PartitionNum"] == 4 and g.Config()["PartitionSize"] == 16513
    assert g.SubConfig(0)["ChunkSize"] == 512 and g.SubConfig(3)["ChunkSize"] == 256
    batch_geometry(g, [(512, 36, 7328)] * 3 + [(256, 68, 5600)])
    for p in range(4):
        a, b = g.SubConfig(p), o.sub(p).Config()
        for k in ("DBSize", "ChunkSize", "SetSize", "MaxQueryNum", "PrimaryHintNum", "MaxQueryPerChunk"):
            assert a[k] == b[k], (p, k)
    ctx.timing_reset()
    g.Preprocessing()
    o.Preprocessing()
    assert_only(ctx, "blk")
    for p in range(4):
        state = g.export_state(p)
        assert hints(state) == (7328 if p < 3 else 5600)
        assert_state(state, o.sub(p).export_state(), E, f"partition {p}")
    rng = np.random.default_rng(N)
    rows = db.reshape(N, E)
    maxq = g.SubConfig(0)["MaxQueryNum"]
    for b in range(int(maxq // (n // 4)) + 8):
        q = rng.integers(0, N, size=n, dtype=np.uint64)
        q[7::11] = q[1]
        got, ok = g.QueryWithMask(q)
        want, _ = o.Query(q)
        assert np.array_equal(got, want), b
        assert np.array_equal(got[ok], rows[q.astype(np.int64)][ok]), b
        assert not got[~ok].any(), b
    sg, so = g.stats(), o.stats()
    for k in ("FinishedBatchNum", "QueriesMadeInPartition", "SupportBatchNum", "PrepCount",
              "LocalStorage", "CommOnline", "CommOffline"):
        assert sg[k] == so[k], k
    assert sg["PrepCount"] == 2   # the sequence crossed one re-preprocessing
    for p in range(4):
        assert_state(g.export_state(p), o.sub(p).export_state(), E, f"partition {p} after the sequence")
    # every fold of the sequence (the re-preprocessing, a partition refilled at its own budget) was the same form
    c = fold_counts(ctx)
    assert c["blk"] >= 2 and c["other"] == c["blk"] and c["rot512"] == c["rot1024"] == c["pipe"] == c["gather"] == 0, c


GROUP_SEEDS = [SEED, 41, 42, 43]


@pytest.mark.parametrize("N,F,SS,H,opt,form", [
    # virtual hint groups mixing the four clients (ngc == 0) / K = 4 in the pipelined fold's XCD order
    pytest.param(80000, 8, 40, 8064, 1, "rot512", id="80000-rot512"),
    pytest.param(80000, 8, 40, 8064, 0, "pipe", id="80000-pipe"),
    # 4,768 hints per partition, fewer than a rotated group's 5,120: one group per client (ngc == 1)
    pytest.param(66400, 1, 36, 4768, 1, "rot512", id="66400-rot512-per-client-groups"),
])
def test_group_fold(ctx, oracle, fold_rot, N, F, SS, H, opt, form):
    """pm_batchpir_group_preprocessing of four clients of one CS-512 server
    (four partitions each) is ONE fold launch of the expected form, and every
    client's state equals an independent oracle client with its seed."""
    import pacmann_amd as pm
    E, B = 8, 8
    fold_rot(opt)
    db = rand_db(N, E, N + E)
    server = pm.SimpleBatchPianoPIR(N, E * 8, B, db, F, seed=SEED, ctx=ctx)
    clients = [server] + [server.Client(sd, pm.Context(0)) for sd in GROUP_SEEDS[1:]]
    fold_rot(-1)   # the clients keep what they were created with
    P = server.Config()["PartitionNum"]
    assert P == 4
    batch_geometry(server, [(512, SS, H)] * 4)
    for c in clients:
        c.Preprocessing()   # epoch 0, one client at a time
    grp = pm.BatchPIRGroup(clients)
    ctx.timing_reset()
    grp.Preprocessing()     # epoch 1: the group's launch set, on the first client's context
    assert_only(ctx, form)
    for c, sd in zip(clients, GROUP_SEEDS):
        o = oracle.SimpleBatchPianoPIR(N, E * 8, B, db, F, seed=sd)
        o.Preprocessing()
        o.Preprocessing()
        assert c.stats()["PrepCount"] == o.stats()["PrepCount"] == 2
        for p in range(P):
            state = c.export_state(p)
            assert hints(state) == H
            assert_state(state, o.sub(p).export_state(), E, f"client seed {sd} partition {p}")


def test_client_of_server_without_image(ctx, oracle, fold_rot):
    """A server created with "fold_rot" 0 has no fold image; a client created
    later, with the option back at its default, goes without one too and folds
    with k_prep_fold_pipe over its own chunk-major table."""
    import pacmann_amd as pm
    N, E, B = 80000, 8, 8
    db = rand_db(N, E, N + E)
    fold_rot(0)
    server = pm.SimpleBatchPianoPIR(N, E * 8, B, db, 8, seed=SEED, ctx=ctx)
    fold_rot(-1)
    cctx = pm.Context(0)
    client = server.Client(77, cctx)
    batch_geometry(client, [(512, 40, 8064)] * 4)
    cctx.timing_reset()
    client.Preprocessing()
    assert_only(cctx, "pipe")
    o = oracle.SimpleBatchPianoPIR(N, E * 8, B, db, 8, seed=77)
    o.Preprocessing()
    for p in range(4):
        assert_state(client.export_state(p), o.sub(p).export_state(), E, f"partition {p}")


@pytest.mark.parametrize("created,later,form", [(1, 0, "rot512"), (0, 1, "pipe")])
def test_fold_form_is_fixed_at_creation(ctx, oracle, fold_rot, created, later, form):
    """The option is read when the engine is created (image built or not,
    chunk-major table allocated or not) and never at launch: changing it before
    Preprocessing() does not change the fold."""
    import pacmann_amd as pm
    N, E, F = 20000, 6, 8
    fold_rot(created)
    g = pm.PianoPIR(N, E * 8, rand_db(N, E, seed=N + E), F, seed=SEED, ctx=ctx)
    assert g.Config()["ChunkSize"] == 512
    fold_rot(later)
    ctx.timing_reset()
    g.Preprocessing()
    assert_only(ctx, form)
    assert_state(g.export_state(), oracle_pir_state(oracle, N, E, F)[1], E)


def test_group_refuses_mixed_image(ctx, fold_rot):
    """Clients created with and without the image cannot be preprocessed as one
    launch set (one form per set); the call fails before any state changes."""
    import pacmann_amd as pm
    N, E, B = 20000, 4, 2
    fold_rot(1)
    server = pm.SimpleBatchPianoPIR(N, E * 8, B, rand_db(N, E, 3), 8, seed=SEED, ctx=ctx)
    assert server.SubConfig(0)["ChunkSize"] == 512
    fold_rot(0)
    bare = server.Client(5, pm.Context(0))
    for c in (server, bare):
        c.Preprocessing()
    grp = pm.BatchPIRGroup([bare, server])
    with pytest.raises(RuntimeError, match="fold image"):
        grp.Preprocessing()
    assert server.stats()["PrepCount"] == bare.stats()["PrepCount"] == 1


def test_fold_rot_option_values():
    import pacmann_amd as pm
    for v in (2, -2, 7):
        with pytest.raises(RuntimeError, match="fold_rot"):
            pm.set_option("fold_rot", v)
    for v in (0, 1, -1):
        pm.set_option("fold_rot", v)
