"""The packed instances of the pair answer (k_answer_p5k / k_answer_pk) against the oracle.

A graph DB whose f32 coordinates all have zero low halves (SIFT's bytes) gets,
beside the packed fold image, a packed row image: row r = the high halves of
its dim coordinate words as half-words, then its m neighbour ids whole.  The
pair answer of a shared step then gathers rows of 2 dim + 4 m bytes in 16-B
segments and expands the coordinate segments when it reduces the slices, so
everything after the gather sees the row the plain kernel leaves.
"host_answer_packed" counts those launches beside "host_path_answer_p5" /
"host_path_answer_p".

Steps.  The kernels are reached only by shared steps with pre-expanded query
sets: np = clients x partitions >= 128 and qn >= 4 sub-queries per (client,
partition) (test_gpu_answer_chain.py).  A graph of out-degree m has m / 2
partitions, so the cases are groups of 128 / (m / 2) sessions of one base with
4 m ids per session: 512 sub-queries per step, the least that takes the chain.
The shape rule (E % 4 == 0, dim % 8 == 0, 2 E = dim + m) makes m a multiple of
8, so a step's np qn sub-queries are always a multiple of 4: no packed step has
an odd count, and the pair kernel's last workgroup never holds one sub-query
alone here (test_gpu_answer_chain.py covers that on plain rows).

Rows per thread.  A row of nseg segments gives a 128-thread workgroup
nsl = 128 / nseg slices; a thread of slice sl gathers rows sl, sl + nsl, ...
of the SetSize in batches of KG rows: KG = 9 in k_answer_p5k (answer_waves 5),
6 in k_answer_pk (6).  SetSize is a multiple of 4 (pir.go:479-514), the
partitions' row counts below end mid-chunk, and where the chunk count is
rounded up to the SetSize the last chunks lie wholly past the partition's end:
their padded row indices (at or beyond the partition's rows) are skipped.

  dim 128, m 32 (E 80; the headline's row: 24 segments, nsl 5, threads 120-127 idle); rows per slice
    SetSize  4: 1 / 1 / 1 / 1 / 0      below one batch, one slice with no row at all
    SetSize 28: 6 / 6 / 6 / 5 / 5      KG 6: exactly one batch, and one row short of it
    SetSize 36: 8 / 7 / 7 / 7 / 7      KG 6: one batch plus one row (and plus two); KG 9: below one batch
    SetSize 44: 9 / 9 / 9 / 9 / 8      KG 9: exactly one batch; KG 6: two batches, the last partial;
                                       43 chunks of rows: chunk 43 is padding
    SetSize 48: 10 / 10 / 10 / 9 / 9   KG 9: one batch plus one row; 47 chunks of rows
    SetSize 60: 12 / 12 / 12 / 12 / 12 KG 9: two batches, the last partial (9 + 3); KG 6: two whole
                                       batches; 59 chunks of rows
  dim 32, m 8 (E 20: 6 segments, nsl 21, threads 126-127 idle)
    SetSize  4: 1 x 4, 0 x 17          most slices of the one batch without a row
    SetSize 40: 2 x 19, 1 x 2          (40 = 21 + 19); the last chunk partial
  dim 24, m 8 (E 16: 3 + 2 segments, nsl 25; dim % 16 == 8: a packed answer over a plain fold image)
    SetSize 40: 2 x 15, 1 x 10

The SIFT1M shape itself (SetSize 124: 25 / 25 / 25 / 25 / 24 rows, three batches of 9 with the
last partial) runs packed in test_gpu_headline.py.
"""
import numpy as np
import pytest

from tests.test_gpu_answer_chain import STATE_KEYS

pytestmark = pytest.mark.gpu

SEED = 20240917
BATCHES = 2
QN = 4
# (dim, m) -> SetSize -> rows per partition (ChunkSize = the power of two >= 2 sqrt(rows))
GEOM = {
    (128, 32): {4: 128, 28: 3500, 36: 9000, 44: 11000, 48: 12000, 60: 15000},
    (32, 8): {4: 128, 40: 20000},
    (24, 8): {40: 20000},
}
SHAPES = [(d, m, ss) for (d, m), by_ss in GEOM.items() for ss in by_ss]

_data, _reference = {}, {}


@pytest.fixture
def options():
    import pacmann_amd as pm
    try:
        yield pm.set_option
    finally:
        pm.set_option("answer_pack", -1)
        pm.set_option("answer_waves", -2)
        pm.set_option("device_loop", -1)


def seeds(m):
    return [(SEED + 31 * i, 5 + i) for i in range(128 // (m // 2))]


def data(dim, m, ss, spoil=None):
    """Integer-valued vectors and a random graph (test_gpu_fold_pack.data), and two batches of ids per
    session; spoil: the value of one coordinate of the DB's last row."""
    key = (dim, m, ss, spoil)
    if key not in _data:
        P = m // 2
        N = P * GEOM[dim, m][ss]
        rng = np.random.default_rng(1000 * ss + dim + m)
        v = rng.integers(0, 256, size=(N, dim)).astype(np.float32)
        g = rng.integers(0, N, size=(N, m)).astype(np.uint32)
        if spoil is not None:
            v[N - 1, dim - 3] = spoil
        ids = rng.integers(0, N, size=(BATCHES, len(seeds(m)), P * QN), dtype=np.uint64)
        ids[:, :, 3] = ids[:, :, 1]          # a repeat inside a batch
        ids[1, :, 0] = ids[0, :, 0]          # an id answered in the batch before: the local cache
        ids[0, 0, 5] = N - 1                 # the DB's last row
        for a in (v, g, ids):
            a.setflags(write=False)
        _data[key] = (v, g, ids)
    return _data[key]


def oracle_run(oracle, dim, m, ss, spoil=None):
    """Every session's responses per batch and its partitions' states after the last one: computed
    once per DB and shared by every case over it."""
    key = (dim, m, ss, spoil)
    if key not in _reference:
        v, g, ids = data(dim, m, ss, spoil)
        want, state, stats = [], [], []
        for i, (ps, s) in enumerate(seeds(m)):
            o = oracle.Graph(v, g, pir_seed=ps, search_seed=s)
            o.Preprocess()
            want.append(np.stack([o.pir().Query(ids[b, i])[0] for b in range(BATCHES)]))
            state.append([o.pir().sub(p).export_state() for p in range(m // 2)])
            stats.append(o.pir().stats())
            del o
        want = np.stack(want, axis=1)   # [batch, session, id, word]
        for a in (want, *[x[k] for st in state for x in st for k in STATE_KEYS]):
            a.setflags(write=False)
        _reference[key] = (want, state, stats)
    return _reference[key]


def sessions(v, g, m):
    import pacmann_amd as pm
    sd = seeds(m)
    base = pm.PIRGraphInfo(v, g, pir_seed=sd[0][0], search_seed=sd[0][1], ctx=pm.Context(0))
    base.Preprocess()
    sess = [base] + [base.Session(p, s, pm.Context(0)) for p, s in sd[1:]]
    for x in sess[1:]:
        x.Preprocess()
    return sess


def run_group(pirs, ctx, ids, ref, forms, packed):
    """Both batches through one BatchPIRGroup of `pirs`: responses, flags, every partition's state and the
    counters of the group's context (the first client's)."""
    import pacmann_amd as pm
    from tests.test_gpu_step_forms import assert_forms
    want, state, stats = ref
    grp = pm.BatchPIRGroup(pirs)
    ctx.timing_reset()
    ctx.timing(2)
    try:
        for b in range(BATCHES):
            got, ok = grp.QueryWithMask(ids[b])
            assert np.array_equal(got, want[b]), b
            assert not got[~ok].any(), b
            assert ok.any(), b
        ctx.sync()
    finally:
        ctx.timing(False)
    launches = {k: ctx.timing_get(k)[0] for k in ("match_resolve", "answer", "step", "hint_match", "gather")}
    assert launches == {"match_resolve": BATCHES, "answer": BATCHES, "step": 0, "hint_match": 0, "gather": 0}
    assert_forms(ctx, BATCHES, forms)
    assert ctx.timing_get("host_answer_packed")[0] == (BATCHES if packed else 0)
    for i, c in enumerate(pirs):
        for key in ("FinishedBatchNum", "QueriesMadeInPartition", "PrepCount"):
            assert c.stats()[key] == stats[i][key], (i, key)
        for p in range(len(state[i])):
            a = c.export_state(p)
            for k in STATE_KEYS:
                assert np.array_equal(a[k], state[i][p][k]), (i, p, k)


def run_sessions(oracle, dim, m, ss, waves, packed=True, spoil=None):
    v, g, ids = data(dim, m, ss, spoil)
    ref = oracle_run(oracle, dim, m, ss, spoil)
    sess = sessions(v, g, m)
    pirs = [x.PIR for x in sess]
    assert pirs[0].Config()["PartitionNum"] == m // 2 and pirs[0].SubConfig(0)["SetSize"] == ss
    assert len(pirs) * (m // 2) * QN == 512
    fold = {k: sess[0].ctx.timing_get("host_fold_" + k)[0] for k in ("rot512p", "rot512")}   # the base's Preprocess
    run_group(pirs, sess[0].ctx, ids, ref, ("mr_s2", "answer_p5" if waves == 5 else "answer_p"), packed)
    return fold


@pytest.mark.parametrize("waves", [6, 5])
@pytest.mark.parametrize("dim,m,ss", SHAPES)
def test_packed_answer_matches_oracle(oracle, options, dim, m, ss, waves):
    """Both packed forms at the SetSizes of the module docstring: two batches per session, each one
    shared step of k_match_resolve_s<2,256> -> the asked-for pair form, every answer launch a packed
    one.  Responses, flags and every partition's refreshed state equal the oracle's bit for bit."""
    options("answer_waves", waves)
    fold = run_sessions(oracle, dim, m, ss, waves)
    if GEOM[dim, m][ss] == 20000:   # ChunkSize 512: the rotated fold, over a packed image only where dim % 16 == 0
        assert fold["rot512p" if dim % 16 == 0 else "rot512"] > 0 and fold["rot512" if dim % 16 == 0 else "rot512p"] == 0, fold


def test_option_off_same_answers(oracle, options):
    """ "answer_pack" 0 when the server is created: the same answers and states from the plain rows."""
    options("answer_pack", 0)
    run_sessions(oracle, 32, 8, 40, 5, packed=False)


@pytest.mark.parametrize("value,packed", [
    pytest.param(0.5, True, id="half"),          # 0x3f000000: not an integer, but nothing the image drops
    pytest.param(1.0 / 3.0, False, id="third"),  # 0x3eaaaaab: the detector must refuse
])
def test_one_coordinate_decides(oracle, options, value, packed):
    """One coordinate of the DB's last row (which the first batch asks for): a non-zero low half
    there alone turns the packed image off, and the answers are the oracle's either way."""
    v, _, _ = data(32, 8, 4, value)
    bits = int(v[-1, 32 - 3].view(np.uint32))
    assert (bits & 0xffff == 0) == packed
    run_sessions(oracle, 32, 8, 4, 5, packed=packed, spoil=value)


@pytest.mark.parametrize("opt", [1, 0])
def test_session_keeps_base_decision(oracle, options, opt):
    """Sessions share their base's image and decision whatever "answer_pack" says when they are created."""
    import pacmann_amd as pm
    dim, m, ss = 32, 8, 4
    v, g, ids = data(dim, m, ss)
    sd = seeds(m)
    options("answer_pack", opt)
    base = pm.PIRGraphInfo(v, g, pir_seed=sd[0][0], search_seed=sd[0][1], ctx=pm.Context(0))
    base.Preprocess()
    options("answer_pack", 1 - opt)
    sess = [base] + [base.Session(p, s, pm.Context(0)) for p, s in sd[1:]]
    for x in sess[1:]:
        x.Preprocess()
    # the group's steps run on the second session's context and server handle: a session's own decision
    order = [1, 0] + list(range(2, len(sess)))
    ref = oracle_run(oracle, dim, m, ss)
    ref = (ref[0][:, order], [ref[1][i] for i in order], [ref[2][i] for i in order])
    run_group([sess[i].PIR for i in order], sess[1].ctx, ids[:, order], ref, ("mr_s2", "answer_p5"), packed=bool(opt))


def test_raw_engine_never_packs(oracle, options):
    """The same rows given to a bare batch PIR engine and its clients: no entry layout, no packed image."""
    import pacmann_amd as pm
    dim, m, ss = 32, 8, 4
    v, g, ids = data(dim, m, ss)
    N = v.shape[0]
    raw = np.concatenate([v.view(np.uint32), g], axis=1).reshape(-1).view(np.uint64)
    ctx = pm.Context(0)
    sd = seeds(m)
    server = pm.SimpleBatchPianoPIR(N, (dim + m) * 4, m, raw, 8, seed=sd[0][0], ctx=ctx)
    clients = [server] + [server.Client(p) for p, _ in sd[1:]]
    for c in clients:
        c.Preprocessing()
    run_group(clients, ctx, ids, oracle_run(oracle, dim, m, ss), ("mr_s2", "answer_p5"), packed=False)


def test_device_loop_on_and_off(options):
    """2 teams x 8 sessions on a 16,384-vertex SIFT-like graph (768 sub-queries per team step over 128
    partitions: k_match_resolve_s -> k_answer_p5k), one query each: the device loop and the host loop
    on fresh sessions with the same seeds give the same answers and counters, every pair answer of
    both a packed one."""
    import pacmann_amd as pm
    from pacmann_amd.synth import random_graph, sift_like_vectors
    from tests.test_gpu_step_forms import form_counts
    n, S = 16384, 16
    v = sift_like_vectors(n, 128, seed=71)
    graph = random_graph(n, 32, seed=72)
    sd = [(80 + i, 90 + i) for i in range(S)]
    rng = np.random.default_rng(75)
    qs = np.stack([np.clip(np.rint(v[rng.integers(0, n, 1)] + rng.normal(0, 8, (1, 128))), 0, 255).astype(np.float32)
                   for _ in sd])
    out = {}
    for mode in (1, 0):
        options("device_loop", mode)
        base = pm.PIRGraphInfo(v, graph, pir_seed=1, search_seed=2, ctx=pm.Context(0))
        base.Preprocess()
        sess = [base.Session(p, s) for p, s in sd]
        for x in sess:
            x.Preprocess()
        for x in sess:
            x.ctx.timing_reset()
        ans, _, _, _ = pm.search_loop_batched(sess, qs, 10, 20, 3, 2, 4)
        ctxs = [x.ctx for x in sess]
        forms = form_counts(ctxs)
        packed = sum(c.timing_get("host_answer_packed")[0] for c in ctxs)
        dev = sum(c.timing_get("host_dev_steps")[0] for c in ctxs)
        out[mode] = (ans, [x.counts() for x in sess], [x.PIR.stats() for x in sess], forms, packed, dev)
    (a1, c1, s1, f1, p1, d1), (a0, c0, s0, f0, p0, d0) = out[1], out[0]
    assert d1 == 20 * 2 and d0 == 0
    assert np.array_equal(a1, a0) and c1 == c0
    for a, b in zip(s1, s0):
        for key in ("FinishedBatchNum", "QueriesMadeInPartition", "PrepCount"):
            assert a[key] == b[key], key
    assert f1["answer_p5"] == 40 and f1["answer_p"] == 0, f1
    assert p1 == f1["answer_p5"] > 0 and p0 == f0["answer_p5"] + f0["answer_p"] > 0, (p1, p0, f1, f0)
