"""k_prep_offsets, every store and AES form it has, against the CPU oracle.

The kernel writes three tables that export_state() does not show directly:
the tag-major tiles (tabT: the fold and the set expansion read them), the hint
search rows (cur) and, where the fold stages it, the chunk-major table (tab).
So every case runs one client's preprocessing and compares the full exported
hint state bit for bit (the parities are folded through tabT or tab), then
sends one batch of queries (the hint search reads cur, the expansion and the
refresh read tabT) and compares every response and the state after it.

What the shapes reach (part_params: SetSize is a multiple of 4, PrimaryHintNum
= ceil(ln 2 (F + 1)) ChunkSize; cur_k: chunk pairs interleaved where
2 PrimaryHintNum <= 128 SetSize; pmk::fold_form for the chunk-major table):

  N, E, F            CS     SS    PH     H       cur  tab  AES form
  16, 4, 0           8      4     8      40      K=2  yes  round 2 per hint
  200, 4, 0          32     8     32     288     K=2  yes  round 2 per hint
  1,500, 4, 8        128    12    896    1,760   K=1  yes  round 2 per hint
  5,000, 6, 8        256    20    1,792  3,712   K=1  yes  round 2 per hint
  62,500, 4, 8       512    124   3,584  12,512  K=2  no   round 2 per hint
  200,704, 8, 8      1,024  196   7,168  24,416  K=2  no   round 2 per hint
  530,433, 4, 0      2,048  260   2,048  31,168  K=2  yes  SetSize > 256
  16,800,000, 4, 0   16,384 1,028 16,384 221,984 K=2  no   SetSize > 256

- SetSize 4, 12, 20, 124, 196, 260, 1,028: not multiples of 8, so the last
  tile is padded with kSkip in place of its missing pairs of chunks.
- H 40: fewer hints than a wave; PH 8 and 32: primary and backup hints in
  one wave; PH 1,792 and 3,584 fall inside a 1,024-thread workgroup; no H is
  a multiple of 1,024.
- Every chunk is the own chunk of Qpc backup hints, so the patch after the
  tile meets the first and the last chunk of a tile and the partial tile.
- ChunkSize 256, 512 and 16,384 (and five more) for the mask of both halves.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20240501
STATE_KEYS = ["round_keys", "primary_tag", "primary_parity", "primary_pp", "backup_tag",
              "backup_parity", "repl_idx", "repl_val", "hist"]

# N, E, F, then the parameters the case is there for: ChunkSize, SetSize, PrimaryHintNum
CASES = [
    (16, 4, 0, 8, 4, 8),
    (200, 4, 0, 32, 8, 32),
    (1_500, 4, 8, 128, 12, 896),
    (5_000, 6, 8, 256, 20, 1_792),
    (62_500, 4, 8, 512, 124, 3_584),
    (200_704, 8, 8, 1_024, 196, 7_168),
    (530_433, 4, 0, 2_048, 260, 2_048),
    (16_800_000, 4, 0, 16_384, 1_028, 16_384),
]


def assert_state_equal(a, b):
    for k in STATE_KEYS:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("N,E,F,CS,SS,PH", CASES, ids=[f"cs{c[3]}_ss{c[4]}" for c in CASES])
def test_prep_offsets_state_and_queries(ctx, oracle, N, E, F, CS, SS, PH):
    import pacmann_amd as pm
    db = np.random.default_rng(N + E).integers(0, 2**64, size=N * E, dtype=np.uint64)
    g = pm.PianoPIR(N, E * 8, db, F, seed=SEED, ctx=ctx)
    o = oracle.PianoPIR(N, E * 8, db, F, seed=SEED)
    cfg = g.Config()
    assert cfg == o.Config()
    assert (cfg["ChunkSize"], cfg["SetSize"], cfg["PrimaryHintNum"]) == (CS, SS, PH)
    g.Preprocessing()
    o.Preprocessing()
    assert_state_equal(g.export_state(), o.export_state())
    # one batch of queries: real and dummy, a repeat, two ids of one chunk
    rng = np.random.default_rng(N)
    ids = rng.integers(0, N, size=min(48, cfg["MaxQueryNum"]))
    ids[5::11] = ids[2]
    ids[7::13] = ids[3] ^ 1
    EX = E & ~3
    for i, idx in enumerate(ids):
        real = (i % 9) != 4
        got, err = g.Query(int(idx), real)
        want, st = o.Query(int(idx), real)
        assert (err.code if err else 0) == st, i
        assert np.array_equal(got, want), i
        if real and st == 0:
            assert np.array_equal(got[:EX], db[idx * E: idx * E + EX])
    assert_state_equal(g.export_state(), o.export_state())
