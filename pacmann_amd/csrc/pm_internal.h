// pm_internal.h — shared host/device definitions for libpacmann.so (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

// Device code sees the state pointers of PmPart / PmStep in the global address
// space, so their accesses lower to global_* instead of flat_* instructions
// (a flat access counts on lgkmcnt too: every later LDS wait would also wait
// for the outstanding global stores of the resolve chain).  Same layout on
// host and device (64-bit pointers).  Host-only translation units (the engine)
// define PM_HOST_TU so their device pass sees the plain host types.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(PM_HOST_TU)
#define PM_G __attribute__((address_space(1)))
#else
#define PM_G
#endif

namespace pm {

constexpr uint32_t kDefaultProgramPoint = 0x7fffffffu;   // pir.go:15
constexpr uint64_t kDefaultValue = 0xdeadbeefULL;        // batch-pir.go:15
constexpr uint16_t kSkip = 0xffffu;                      // prep offset sentinel: backup hint's own chunk
constexpr int kBlock = 256;

// Randomness streams; identical spec to oracle/pm_oracle.cpp.
enum : uint64_t { DOM_KEY = 1, DOM_REPL = 2, DOM_DUMMY = 3, DOM_SYNTH_DB = 9, DOM_SYNTH_VEC = 10, DOM_SYNTH_NB = 11 };
__host__ __device__ inline uint64_t sm64(uint64_t x) {
  uint64_t z = x + 0x9e3779b97f4a7c15ULL;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t hash4(uint64_t seed, uint64_t dom, uint64_t a, uint64_t b,
                                          uint64_t c) {
  uint64_t h = sm64(seed + dom);
  h = sm64(h ^ a);
  h = sm64(h ^ b);
  return sm64(h ^ c);
}

// The synthetic graph DB (pm_graph_create_synth; BIGANN-scale configs[3]/[4],
// where no graph can be built or shipped): the reference's synthetic mode
// (private-search.go:114-117,168-170: genRandomMatrix's uniform [0,1) f32
// vectors, genRandomGraph's uniform neighbour ids without self loops,
// :42-69) as a pure function of (seed, vertex), so a shard generates only its
// own rows and anyone can recompute any row.  u32 element e of vertex v's
// PIRGraphInfo entry (private-search.go:363-397: f32[dim] || u32[m]):
//   e <  dim: float((sm64(kv ^ (v*dim + e)) >> 40) * 2^-24)        (24 random bits, rand.Float32)
//   e >= dim: x = sm64(kg ^ (v*m + k) ^ (a << 56)) % n for a = 0, 1, ... until
//             x != v (k = e - dim; genRandomGraph redraws a self loop, so the
//             neighbours are uniform over the other n - 1 vertices)
// with kv = sm64(seed + DOM_SYNTH_VEC), kg = sm64(seed + DOM_SYNTH_NB).
__host__ __device__ inline float graph_synth_vec(uint64_t kv, uint64_t v, uint32_t dim, uint32_t j) {
  return (float)(sm64(kv ^ (v * dim + j)) >> 40) * 0x1.0p-24f;
}
__host__ __device__ inline uint32_t graph_synth_nb(uint64_t kg, uint64_t n, uint64_t v, uint32_t m, uint32_t k) {
  const uint64_t c = v * m + k;
  uint64_t x = sm64(kg ^ c) % n;
  for (uint64_t a = 1; x == v; ++a) x = sm64(kg ^ c ^ (a << 56)) % n;   // n > 1 (pm_graph_create_synth)
  return (uint32_t)x;
}
__host__ __device__ inline uint32_t graph_synth_elem(uint64_t kv, uint64_t kg, uint64_t n, uint32_t dim, uint32_t m,
                                                     uint64_t v, uint32_t e) {
  if (e < dim) return __builtin_bit_cast(uint32_t, graph_synth_vec(kv, v, dim, e));
  return graph_synth_nb(kg, n, v, m, e - dim);
}

// One PianoPIR instance ("partition") as the device sees it.  Parameters
// follow NewPianoPIR / NewPianoPIRClient (pir.go:130-175, 479-514).
// Hint index space h in [0, H): h < PH primary hints, h >= PH backup hint
// (g, j) with h = PH + g*Qpc + j (backupShortTag[g][j], pir.go:244-251).
struct PmPart {
  uint64_t N;        // DBSize of this sub-PIR
  uint64_t row0;     // first global DB row of this partition
  uint64_t seed;     // randomness seed (keys, replacement, dummy)
  uint64_t epoch;    // preprocessing epoch in use
  uint64_t idx;      // partition index (stream domain)
  uint32_t CS, log2CS, SS, PH, Qpc, H, MaxQ, curk;   // curk: chunks per hint-search block (cur_index)
  uint32_t rk[44];   // expanded AES-128 key (expandKeyAsm layout)
  // client state, device-resident
  PM_G uint32_t* tag;     // [H]   short tags (primary tags mutate on refresh)
  PM_G uint32_t* pp;      // [PH]  primaryProgramPoint
  PM_G uint64_t* parity;  // [H*E] primary parities then backup parities
  PM_G uint32_t* ridx;    // [SS*Qpc] replacementIdx
  PM_G uint64_t* rval;    // [SS*Qpc*E] replacementVal
  PM_G uint32_t* hist;    // [SS]  QueryHistogram
  PM_G uint32_t* fqn;     // [1]   FinishedQueryNum
  PM_G uint64_t* arena;   // [MaxQ*E] localCache rows (pir.go:120), slot = FinishedQueryNum at answer time
  // PRF table (only where the fold reads it, pmk::fold_needs_tab; else null):
  // tab[c*H + t] = PRF(tag t, chunk c) & (CS-1) for every tag t in
  // [0, H) and chunk c in [0, SS) (kSkip at a backup tag's own chunk).  Every
  // tag a hint can carry is a hint index (primary tags start at h, a refresh
  // hands over backup tag PH+g*Qpc+j), so this table, built once per
  // preprocessing, holds every PRF value the online phase needs.
  PM_G uint16_t* tab;
  PM_G uint16_t* tabT;    // the same table tag-major in tiles of 8 chunks (tabT_at): set expansion
                          // reads one tag's row; k_prep_offsets writes whole 16-B tiles
  // The hint search's table: entry (c, h) = PRF(current tag of primary hint
  // h, chunk c) & (CS-1), i.e. tab[c][tag[h]] kept in hint order, so matching
  // a (chunk, offset) streams chunk c's row of PH u16 instead of gathering
  // through the tags.  k_prep_offsets seeds it (tags are h); the final refresh
  // of a hint in a step rewrites its column from tabT[new tag] (pm_query.hip
  // refresh_cur).  Layout cur_index: chunk pairs interleaved in 16-B blocks.
  PM_G uint16_t* cur;
  // the search query this client's decoded rows are scored against (L2) when
  // several clients' steps share one launch (pm_search_loop_batched); null:
  // the step's PmStep::q
  const PM_G float* qv;
  // The partition's fold image (server-side, built once with the DB; null
  // where k_prep_fold_rot does not apply): per 32-B column slice s and group
  // of NCH chunks b (4 at CS 512, 2 at CS 1,024), the 64 KB LDS image
  // k_prep_fold_rot stages, line k = row k of chunks NCH b .. (rows past N
  // zero).  pmk::fold_image_words.  Packed (FOLD_ROT512P): the coordinate
  // slices hold high halves only, 16 words per slice (k_fold_image).
  const PM_G uint64_t* img;
};
// The server's side of a partition, all that k_server_answer_parts reads of it
// (pm_batchpir_server_answer): fixed when the handle is created, no client state.
struct PmSrvPart {
  uint64_t N;      // DBSize of this sub-PIR
  uint64_t row0;   // its first row in the handle's DB
  uint32_t CS, SS;
};

// tabT layout: chunk c of tag t at tile (c / 8, t), element c % 8 (16-B tiles of
// 8 chunks; SetSize padded to a multiple of 8 with kSkip), so the writer of 8
// chunks x consecutive tags stores full lines instead of one 2-B store per line.
__host__ __device__ inline uint64_t tabT_index(uint32_t H, uint32_t t, uint32_t c) {
  return ((uint64_t)(c >> 3) * H + t) * 8 + (c & 7);
}
// where a 16-B item of a fold image comes from (k_fold_image, fold_image_src)
struct FoldImageSrc { uint64_t row; uint32_t word; bool packed; };
__host__ __device__ inline uint64_t tabT_words(uint32_t H, uint32_t SS) { return (uint64_t)((SS + 7) / 8) * 8 * H; }

// Hint-search table layout: [SS / 2][PH8 / 8][2][8] u16 (PH8 = PH rounded up
// to 8): block b of chunk c's row (hints 8b .. 8b + 7, one 16-B load) sits
// beside the same block of chunk c ^ 1.  A refresh writes a hint's entry of
// every chunk, i.e. one column: paired, its SS entries touch SS / 2 cache lines
// instead of SS (random line writes cost ~2.6 random line reads on MI355X:
// tools/gather_bench.hip regw_*), while a row's reads stay whole 16-B blocks
// (every other one: twice the row's bytes through L2).
#ifndef PM_CUR_K
#define PM_CUR_K 0   // chunks interleaved per 16-B hint block: 0 = chosen per partition (cur_k), else forced
#endif
// K chunks interleaved: a refresh writes SS / K lines, a search reads K x its
// row.  K = 2 unless the row (PH x 2 B) outweighs the column's lines (SS x
// 128 B): BIGANN-100M's 57,344-hint rows read twice cost the hint search more
// than the halved refresh saves (k_match_part8 34 -> 55 us per team step)
__host__ __device__ inline uint32_t cur_k(uint32_t PH, uint32_t SS) {
  return PM_CUR_K ? PM_CUR_K : ((uint64_t)PH * 2 > (uint64_t)SS * 128 ? 1u : 2u);
}
__host__ __device__ inline uint32_t cur_blocks(uint32_t PH) { return (PH + 7) >> 3; }
__host__ __device__ inline uint64_t cur_index(uint32_t PH, uint32_t K, uint32_t c, uint32_t h) {
  return K == 2 ? (((uint64_t)(c >> 1) * cur_blocks(PH) + (h >> 3)) * 2 + (c & 1)) * 8 + (h & 7)
                : (((uint64_t)(c / K) * cur_blocks(PH) + (h >> 3)) * K + (c % K)) * 8 + (h & 7);
}
// chunk c's row: hint h at row[cur_row_off(K, h)], block b (8 hints) at row + 8 K b
__host__ __device__ inline uint64_t cur_row(uint32_t PH, uint32_t K, uint32_t c) { return cur_index(PH, K, c, 0); }
__host__ __device__ inline uint32_t cur_row_off(uint32_t K, uint32_t h) { return (h >> 3) * 8 * K + (h & 7); }
__host__ __device__ inline uint64_t cur_words(uint32_t PH, uint32_t SS, uint32_t K) {
  return (uint64_t)((SS + K - 1) / K) * cur_blocks(PH) * 8 * K;
}

// Sub-query kinds / statuses for one batched step.
enum : uint32_t { SUB_NONE = 0, SUB_REAL = 1, SUB_DUMMY = 2, SUB_HOSTCACHE = 3 };
enum : uint32_t {
  ST_OK = 0, ST_EBUDGET = 1, ST_ECHUNK = 2, ST_ENOHIT = 3, ST_ERANGE = 4,
  ST_DUMMY = 8, ST_CACHED = 9, ST_DUP = 10, ST_SKIP = 11
};
struct PmSub {
  uint32_t part, kind;
  uint64_t idx;   // REAL: local index; DUMMY: dummy counter; HOSTCACHE: arena slot
};
// Per-sub-query resolution record written by k_resolve.
struct PmRes {
  uint32_t status, hit, chunk, ing;   // ing = in-group index (QueryHistogram before)
  uint32_t tag, pp;                   // hit hint's tag / program point used for the expansion
  uint32_t slot;                      // OK: arena slot; CACHED: arena slot; DUP: earlier sub
  uint32_t flags;                     // bit 0: hint refreshed earlier in this step (chained);
                                      // bit 1: a later sub-query in this step re-hits this hint
};
// Per-sub-query result header, written by the GPU into pinned host memory
// after the sub-query's row.  Stores to fine-grained host memory reach the
// host in no guaranteed order (measured: ~3e-5 of rows not yet complete when
// their token is first seen), and ordering them inside the kernel costs
// 2.8-4.4x the answer kernel's time (a system-scope L2 write-back per
// workgroup, or write-through stores).  So the token only says "answered";
// the host takes a step's results after the step's completion event, recorded
// with a system-scope release after the last kernel (pm_engine.cpp
// wait_step), which orders every byte.  The header also carries a
// multilinear hash of the row words the host reads ([pf_w0, pf_w1) of PmStep):
//   csum = token * kCsumMix + sum_w row[w] * row_hash_mult(w)   (mod 2^64)
// with odd multipliers, checked after completion as an assertion (and, with
// PM_PUBLISH_WAIT=0, as the token-time acceptance test: one stale word changes
// the sum by (new - old) * odd != 0; a stale header never matches).
constexpr uint64_t kCsumMix = 0x9E3779B97F4A7C15ull;
__host__ __device__ inline uint64_t row_hash_mult(uint64_t w) { return sm64(w ^ 0x5851F42D4C957F2Dull) | 1ull; }
struct alignas(16) PmOutHdr {
  uint32_t status, ref;
  float dist;
  uint32_t token;
  uint64_t csum, pad;
};
// Arguments of the step kernels (pm_query.hip).
#ifndef PM_KARG_SUBS
#define PM_KARG_SUBS 112
#endif
constexpr uint32_t kArgSubs = PM_KARG_SUBS, kArgParts = PM_KARG_SUBS > 1 ? 32 : 1;
// k_step gather helpers (PmStep::nhelp): at most kStepHelpMax per sub-query,
// for entries of <= 256 gathered words; granules per helper: 2 x 256 partial
// words + 8 guess fields
constexpr uint32_t kStepHelpMax = 3, kHelpWords = 256, kHelpGran = 2 * kHelpWords + 8;
struct PmStep {
  const PM_G PmPart* parts;
  const PM_G PmSub* subs_h;    // pinned host descriptor, read zero-copy by k_match
  const PM_G uint32_t* sb_h;   // sub_begin[np+1] (pinned host)
  PM_G PmSub* subs;            // device copies
  PM_G uint32_t* sb;
  PM_G uint64_t* bits;         // [nsub][words] hint-match bits (k_match -> k_resolve)
  PM_G uint32_t* cand;         // [nsub][cblk][6]: per k_match block its first two matches
                               // {hint, tag, program point} x 2 (hint kNone: none)
  PM_G PmRes* res;             // [nsub]
  PM_G uint64_t* ans;          // [nsub][E] raw answers of chained sub-queries
  PM_G uint32_t* done;         // [0..1] step completion counter (chain_add, pm_query.hip),
                               // [2] chained sub-queries, [3..] their list (filled by the
                               // resolvers; re-armed by each step's finisher)
  const PM_G uint64_t* db;
  // The server's packed row image for k_answer_p5k / k_answer_pk (pmk::answer_pack_image; null: none):
  // row r = the high halves of db row r's 8 pk_cseg coordinate words as half-words, then its other
  // 32-bit words whole; pk_nseg 16-B segments per row, the first pk_cseg of them coordinates
  const PM_G uint64_t* dbp;
  uint32_t pk_nseg, pk_cseg;
  const PM_G float* q;         // search query (device) or null
  PM_G PmOutHdr* hdr_h;        // pinned host outputs
  PM_G uint64_t* rows_h;
  PM_G uint64_t* stamps;       // PM_STAMPS diagnostic builds only: s_memtime per phase
  PM_G uint32_t* meta;         // [nsub][2]: chunk QueryHistogram, predicted in-chunk index
  PM_G uint32_t* spec;         // [nsub][64]: predicted re-evaluation values (k_match -> k_resolve)
  // k_step hand-off granules {value, token} (pm_query.hip put_g / get_g)
  PM_G uint64_t* recg;         // [kArgSubs][8] match record + prediction per sub-query
  PM_G uint64_t* specg;        // [kArgSubs][64] predicted re-evaluation values
  PM_G uint64_t* bitsg;        // [kArgSubs][words][2] match bits
  PM_G uint64_t* resg;         // [kArgSubs][8] resolution records
  // k_step gather helpers: nhelp extra workgroups per sub-query each gather a
  // range of the guessed set and hand over its partial XOR (granules: 2 per
  // word of the partial, then the guess fields); 0 = none
  PM_G uint64_t* helpg;        // [kArgSubs][kStepHelpMax][kHelpGran]
  uint32_t nhelp;
  // "step_help_spoil" (tests): helper j (1..3) whose bit j - 1 is set gathers and hands over its partial as
  // usual but publishes kNone as its guessed mode, so the answer refuses every helper's partial and redoes
  uint32_t help_spoil;
  // k_step's speculation record (contexts created with PM_STEP_SPEC=1; null: none): one word per
  // sub-query, stored by its answer workgroup once it knows whether its speculative work stands
  // (step_spec_word below), zeroed before the launch
  PM_G uint32_t* specrec;      // [kArgSubs]
  PM_G uint32_t* err_h;       // pinned host: set when a hand-off spin timed out        // [np] k_step: token of the step whose results the resolver published
  uint32_t words, E, dim, nsub, np, cblk;
  uint32_t np_live;            // partitions with at least one sub-query in this step
  uint32_t pf_w0, pf_w1;       // row words the host reads (PmOutHdr::csum covers them)
  uint32_t rows_partial;       // 1: only words [pf_w0, pf_w1) of each result row are written to the host
  uint32_t no_guess;           // k_step diagnostics: answers wait for their resolution (PM_NO_GUESS=1)
  // Split gather (three-kernel path, wide sets): k_gather writes nsplit partial
  // XORs of each sub-query's set, [nsub][nsplit][E&~3]; k_answer folds them.
  uint32_t nsplit;             // 0/1: k_answer gathers its set itself
  PM_G uint64_t* part_x;
  // Query sets expanded by k_match_resolve_s ([nsub][qw] u16 offsets; qw = SetSize
  // rounded up to 8), read by k_answer with the resolution record; null: the
  // answer expands its set from tabT itself.
  PM_G uint16_t* qset;
  uint32_t qw;
  // Small steps ship the descriptor inside the kernel arguments (no PCIe
  // round trip); larger ones use subs_h / sb_h.
  uint32_t args_valid;
  uint32_t token;              // written into every PmOutHdr of this step
  uint32_t sb_a[kArgParts + 1];
  PmSub subs_a[kArgSubs];
};

// A word of k_step's speculation record (PmStep::specrec; pm_batchpir_step_spec returns them):
//   bits 0-2  the guessed answer mode (step_guess): 1 A_FINAL, 4 A_DUMMY, 7 no guess
//   bit  3    helped: the guess was gathered with the helpers (nhelp > 0 and a guess of A_FINAL / A_DUMMY)
//   bit  4    help_ok: every helper's guess was the answer's (set where not helped)
//   bit  5    kept: the resolution equals the guess in every field the answer reads
//   bit  6    redo: the set was gathered again for the resolution (= !kept || !help_ok)
//   bits 8-10 the resolution's answer mode (answer_mode): 0 A_ZERO, 1 A_FINAL, 2 A_CHAINED, 3 A_CACHED, 4 A_DUMMY
//   bit  31   written (a word the step's kernel never stored reads 0)
__host__ __device__ inline uint32_t step_spec_word(uint32_t gmode, bool helped, bool help_ok, bool kept, bool redo,
                                                   uint32_t mode) {
  return (gmode & 7u) | (helped ? 8u : 0u) | (help_ok ? 16u : 0u) | (kept ? 32u : 0u) | (redo ? 64u : 0u) |
         ((mode & 7u) << 8) | 0x80000000u;
}

// ---- the device-resident team round (pm_drl.hip; pm_search_loop_batched's
// device loop): a lock-step team's 20 rounds of SearchKNN +
// SimpleBatchPianoPIR.Query bucketing run on the GPU, chained on the team's
// stream, with the host touching only a query's start and end.
// the device loop's open-addressing tables (pm_drl.hip; the host builds the
// localCache table with the same probe sequence)
__host__ __device__ inline uint32_t drl_hash(uint32_t k) {
  uint64_t x = k;
  x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33;
  return (uint32_t)x;
}
struct DrlSess {          // one session's search state between launches
  uint64_t rng;           // SplitMix state (the host's id stream, SplitMix::next)
  uint64_t succ;          // successQueryNum (private-search.go:483-497)
  uint32_t nknown, nheap; // knownVertices / the min-heap's sizes
  uint32_t pad0, pad1;
};
enum : uint32_t { DRL_BEGIN = 0, DRL_MID = 1, DRL_END = 2 };
struct DrlArgs {
  uint32_t S, P, qn, n, m, parallel, k, E, dim, kcap, cmask, ns, mode, q, qi, seq;
  uint32_t vec16;                 // rows and neighbour lists 16-B aligned, m / 4 a power of two (vector decode)
  uint64_t N, PS;
  const PmOutHdr* hdr;            // the last shared step's results [nsub] (device)
  const uint64_t* rows;           // ... and rows [nsub][E] (the neighbour words only)
  PmSub* subs;                    // the next shared step's descriptor [S][P][qn]
  uint64_t* gid;                  // ... each sub-query's global id (~0: dummy)
  const uint32_t* graph;          // [N][m] the true neighbour lists (success check, start set)
  const float* start_dist;        // [S][ns] the start set's L2 distances to the query
  const uint32_t* start_ids;      // [S][ns]
  DrlSess* sess;                  // [S]
  uint64_t* dummy;                // [S][P] dummy-query counters (PartHost::dummy_ctr)
  uint32_t* batch;                // [S][n] the round's ids
  uint64_t* heap;                 // [S][kcap] {dist f32 bits | known slot << 32}
  uint64_t* ktab;                 // [S][2 kcap] knownVertices: {id + 1 | slot << 32}, 0 empty
  uint32_t* knb;                  // [S][kcap][m] known vertices' neighbour lists
  float* kdist;                   // [S][kcap]
  uint32_t* kid;                  // [S][kcap]
  uint64_t* const* ctab;          // [S] -> [P][cmask + 1] localCache: {local idx + 1 | arena slot << 32}
  int64_t* answers;               // [S][q][k]
  const double* part_bytes;       // [P] algorithmic answer bytes of one sub-query
  double* step_bytes;             // [launch seq][S] (timing runs; null: not counted)
  uint32_t* step_real;            // [launch seq][S] real sub-queries (timing runs)
  uint64_t* stamps;               // diagnostics (PM_DRL_STAMPS): [16] summed shader clocks per phase of MID rounds
};

// ---- the batched non-private search (pm_knnb.hip; pm_search_knn_batch,
// DESIGN.md §6.5): one workgroup runs a whole SearchKNN of one query over the
// device's vectors and graph, its state in LDS.
struct KnbArgs {
  const float* vec;        // [n][dim]
  const uint32_t* graph;   // [n][m], every id < n
  const uint32_t* start;   // [ns] the start set (GetStartVertex)
  const float* queries;    // [nq][dim]
  uint32_t nq, ns, dim, m, k, max_step, parallel, kcap;
  int64_t* ids;            // [nq][k] top k by (distance, id), -1 padded
  int64_t* steps;          // [nq][k] their reach steps
  uint32_t* needs_host;    // [nq] 1: a pop found the heap empty (the id stream is the host's)
};

}  // namespace pm

// Kernel launchers (pm_kernels.hip).  All asynchronous on `st`.
namespace pmk {
using namespace pm;
void prep_init(hipStream_t st, const PmPart* dparts, int nparts, uint32_t maxH, uint32_t maxRepl,
               uint32_t E, bool zero_state);
void prep_offsets(hipStream_t st, const PmPart* dparts, int nparts, uint32_t maxH, uint32_t maxSS);
// the PRF tables' AES form: 0 = T-table (k_prep_offsets, default), 1 = bitsliced on the
// VALU (k_prep_offsets_bs, pm_aes_bs.h; profiles/r06/aes: 0.93x), -1 = PM_AES_BS's value
void set_aes_bs(int v);
// dparts: `clients` clients of each partition, partition-major (nparts = partitions x clients)
// returns the fold form launched (FOLD_*)
// The forms of the hint fold: the unblocked gather k_prep_fold<W> (odd E, E < 4,
// chunks too wide for LDS), the bank-rotated k_prep_fold_rot<512 / 1024> over
// the fold image, the pipelined k_prep_fold_pipe (one ChunkSize of 512, 1,024
// or 2,048 and no image) and the double-buffered k_prep_fold_blk<8 / 4 / 2>.
// FOLD_ROT512P is k_prep_fold_rot<512> over a packed image: the DB is a graph
// DB whose coordinate words (f32 holding small integers, e.g. SIFT's bytes) all
// have zero low halves, so the image and the fold leave those halves out.
// FOLD_ROT512Q is the same kernel over a bit-packed image: such a DB whose
// coordinates are f32 holding 0..255 and / or whose ids are below 2^20 also has
// constant exponent, sign and high id bits, which the image leaves out too.
enum : int { FOLD_GATHER = 0, FOLD_ROT512 = 1, FOLD_ROT1024 = 2, FOLD_PIPE = 3, FOLD_BLK = 4, FOLD_ROT512P = 5, FOLD_ROT512Q = 6 };
// The one selection of the form: from the partitions' ChunkSize range, the entry
// words, whether the engine was created with a fold image and the image's packed
// coordinate slices (npk, 0: a plain image) or bit-packed fields (qf, 0: none).
// prep_fold dispatches on it and fold_needs_tab follows from it.
int fold_form(uint32_t minCS, uint32_t maxCS, uint32_t E, bool have_img, uint32_t npk = 0, uint32_t qf = 0);
// "fold_rot": 1 / 0 the rotated fold and its image for engines created from now
// on, -1 = PM_FOLD_ROT's value (default on).  Consulted by fold_image_ok only,
// i.e. when an engine is created; an existing engine keeps its form.
void set_fold_rot(int v);
int prep_fold(hipStream_t st, const PmPart* dparts, int nparts, uint32_t maxH, const uint64_t* db,
              uint32_t E, uint32_t minCS, uint32_t maxCS, const uint64_t* zero16, uint32_t clients = 1,
              bool have_img = false, uint32_t minH = 0, uint32_t npk = 0, uint32_t qf = 0);
void prep_repl(hipStream_t st, const PmPart* dparts, int nparts, uint32_t maxRepl,
               const uint64_t* db, uint32_t E);
// The streamed preprocessing (pm_stream.hip; pm_batchpir_prep_stream_rows): UpdatePreprocessing of chunks
// [c0, c0 + nc) of partition parts[part] from `win`, the nrows existing rows of those chunks (row i of win =
// partition row c0 * CS + i; nothing at or past nrows is read).  stream_fold XORs the window's selected rows
// into the parities (read-modify-write; nothing is launched for E < 4 or an empty window); stream_repl
// writes the window's replacement indices and values.  H, Qpc: the partition's.
void stream_fold(hipStream_t st, const PmPart* parts, uint32_t part, uint32_t H, const uint64_t* win, uint32_t c0,
                 uint32_t nc, uint32_t nrows, uint32_t E);
void stream_repl(hipStream_t st, const PmPart* parts, uint32_t part, uint32_t Qpc, const uint64_t* win, uint32_t c0,
                 uint32_t nc, uint32_t nrows, uint32_t E);
// The bank-rotated fold's DB image (CS 512 / 1,024, even E, E >= 4): whether an
// engine being created should have one (the shape fits and "fold_rot" /
// PM_FOLD_ROT allows it; not to be asked at launch time, see fold_form), its
// size per partition (words) and the build of one partition's image.
bool fold_image_ok(uint32_t minCS, uint32_t maxCS, uint32_t E);
// whether the fold of these shapes reads the chunk-major PRF table PmPart::tab
// (otherwise it is not allocated: every other reader uses tabT)
bool fold_needs_tab(uint32_t minCS, uint32_t maxCS, uint32_t E, bool have_img);
uint64_t fold_image_words(uint32_t SS, uint32_t E, uint32_t CS, uint32_t npk = 0, uint32_t qf = 0);
void fold_image(hipStream_t st, uint64_t* img, const uint64_t* part_rows, uint64_t N, uint32_t SS, uint32_t E,
                uint32_t CS, uint32_t npk = 0, uint32_t qf = 0);
// The packed image.  fold_pack_shape: the packed coordinate slices of entries of
// E words whose first `dim` 32-bit words are coordinates (16 per slice), 0 where
// they do not fill whole slices of the folded words.  fold_pack_slices: the same
// for an engine being created, 0 also unless its fold is FOLD_ROT512 and
// "fold_pack" / PM_FOLD_PACK (1 / 0, -1 the environment's, default on) allows
// it.  "fold_bits" / PM_FOLD_BITS (the same values, default on) allows the
// bit-packed image on top of it; off, such a DB takes the packed image.
// row_bits_or: one reduction over the packed DB rows for the bits the images
// leave out: kRowLowHalf if the low half of a coordinate word is not zero,
// kRowCoordBits if a coordinate's sign is set or its exponent bits 6..3 are not
// all equal, kRowIdBits if a later word has a bit above 19 set (flag: 4 device
// bytes; every flag on a HIP error).  fold_bits_form: the bit-packed image's
// fields for a DB with those flags whose packed image has npk slices (w1 | w2
// << 8 | dim / 4 << 16: 12- or 16-bit coordinate and 20- or 32-bit id fields),
// 0 where none has fewer slices or "fold_bits" is off; fold_bits_slices: its
// slices.  All are asked once, when a server packs its DB.
enum : uint32_t { kRowLowHalf = 1, kRowCoordBits = 2, kRowIdBits = 4 };
void set_fold_pack(int v);
void set_fold_bits(int v);
uint32_t fold_pack_shape(uint32_t E, uint32_t dim);
uint32_t fold_pack_slices(uint32_t minCS, uint32_t maxCS, uint32_t E, uint32_t dim);
uint32_t row_bits_or(hipStream_t st, const uint64_t* rows, uint64_t nrows, uint32_t E, uint32_t dim, uint32_t* flag);
uint32_t fold_bits_form(uint32_t E, uint32_t dim, uint32_t npk, uint32_t flags);
uint32_t fold_bits_slices(uint32_t qf, uint32_t E);
// The answer's packed row image (k_answer_p5k / k_answer_pk): for the same kind of
// DB, a row-major copy of the rows without the coordinates' low halves: row r =
// the high halves of its `dim` coordinate words as consecutive half-words, then
// its 2E - dim other 32-bit words whole (2 dim + 4 (2E - dim) bytes; SIFT1M: 384
// instead of 640).  answer_pack_shape: the row's 16-B segments, 0 where the
// entries do not qualify (a graph DB, E % 4 == 0 so that the gather's E & ~3 rule
// cuts nothing, E <= 256, dim % 8 == 0: whole segments of eight half-words, and
// then a stride of whole segments).  answer_pack_segs: the same for a server
// being created, 0 also unless "answer_pack" / PM_ANSWER_PACK (1 / 0, -1 the
// environment's, default on) allows it; read there and nowhere later.
void set_answer_pack(int v);
uint32_t answer_pack_shape(uint32_t E, uint32_t dim);
uint32_t answer_pack_segs(uint32_t E, uint32_t dim);
void answer_pack_image(hipStream_t st, uint64_t* img, const uint64_t* rows, uint64_t nrows, uint32_t E, uint32_t dim);
// k_fold_image's index map on the host (pm_fold_image_map): for image items
// [x0, x0 + n) of a partition, the row, its first 32-bit word and whether the
// item packs the high halves of 8 words (else it holds 4 whole words)
void fold_image_map(uint32_t CS, uint32_t SS, uint32_t npk, uint64_t x0, uint64_t n, uint64_t* row, uint32_t* word,
                    uint8_t* packed);
// Timing events carried by a launch's own dispatch packet (null: untimed)
struct PmEvents { hipEvent_t a = nullptr, b = nullptr; };
// pm_set_option: the hint-search path selectors ("match_part" -1 auto / 0 / 1,
// "match_part8" 0 / 1, "match_resolve" 0 / 1 / 2); -2 restores the environment's
// choice (PM_MATCH_PART, PM_MATCH_PART8, PM_MATCH_RESOLVE).  Returns -1 for an
// unknown name.
int set_option(const char* name, int value);
// The selectors' values for one step: pm_set_option's overrides over the environment's choices, each
// read once per process (PM_MATCH_PART -1, PM_MATCH_PART8 1, PM_MATCH_RESOLVE 1, PM_ANSWER_WAVES 0,
// PM_ANSWER_NT 128, PM_ANSWER_PAIR 1, PM_GATHER_SPLIT 0, PM_STEP_HELP 3; "step_help" 0..3 overrides the
// last, "step_help_spoil" has no variable and is 0 unless set).  One snapshot per step, so a
// pm_set_option on another thread cannot split a step between two paths.
struct StepOpts { int match_part, match_part8, match_resolve, answer_waves, answer_nt, answer_pair, gather_split, step_help, step_help_spoil; };
StepOpts step_opts();
uint32_t step_match_blocks(uint32_t maxPH);   // k_match workgroups per sub-query
// Who builds the step: an engine's own step (engine_step: the device copies of
// the descriptor differ from the host-visible one), a group's shared step
// (group_step: a descriptor too large for the kernel arguments is DMA'd and is
// then its own device copy) or the device loop's (built on the device).
enum : int { STEP_ENGINE = 0, STEP_SHARED = 1, STEP_DEVICE = 2 };
// Small steps ship the descriptor inside the kernel arguments (PmStep::args_valid).
inline bool step_args_fit(uint32_t nsub, uint32_t np) { return nsub <= kArgSubs && np <= kArgParts; }
// What the choice of a step's kernels depends on, and nothing else.
struct StepShape {
  uint32_t np, nsub, np_live, max_per_part, maxPH, maxSS, E;
  bool ph8;           // every partition's PH is a multiple of 8 (k_match_part8, k_match_resolve_s)
  // descriptor facts (of_caller)
  bool args_valid;    // the descriptor travels in the kernel arguments (PmStep::subs_a / sb_a)
  bool desc_shared;   // PmStep::subs == subs_h and sb == sb_h: the kernels' descriptor is in device memory
  bool granules;      // k_step's hand-off granules and error word exist
  // context switches
  bool unfused;       // PM_NO_FUSE or PM_DEBUG_SYNC
  bool no_split, no_guess;
  void of_caller(int kind, bool have_granules) {
    args_valid = kind != STEP_DEVICE && step_args_fit(nsub, np);
    desc_shared = kind == STEP_DEVICE || (kind == STEP_SHARED && !args_valid);
    granules = kind == STEP_ENGINE && have_granules;
  }
};
// The kernels of a step: the hint search (MATCH_*, counted in "host_path_match*")
// and the forms of the others (FORM_*: the one record of which instance
// answered, pm_ctx::step_counter, "host_path_*"): k_step<W>; k_resolve<true>
// / <false>; k_match_resolve_s<2,256> / <4,256> / k_match_resolve; k_gather<W>;
// k_answer_p5 / k_answer_p / k_answer_s<W,NT> / k_answer<W>.
enum : int { MATCH_SUB = 0, MATCH_PART = 1, MATCH_PART8 = 2 };
enum : int { FORM_STEP = 0, FORM_RESOLVE_LDS, FORM_RESOLVE_G, FORM_MR_S2, FORM_MR_S4, FORM_MR_GENERAL,
             FORM_GATHER, FORM_ANSWER_P5, FORM_ANSWER_P, FORM_ANSWER_S, FORM_ANSWER_G, FORM_COUNT };
// A step's launches in order: FUSED alone, or MR or MATCH + RESOLVE, then GATHER (split sets), then ANSWER.
enum : int { STAGE_FUSED = 0, STAGE_MR, STAGE_MATCH, STAGE_RESOLVE, STAGE_GATHER, STAGE_ANSWER, STAGE_COUNT };
struct StepLaunch { int form = -1; uint32_t gx = 0, gy = 1, block = 0; };   // form < 0: not launched; MATCH_* at STAGE_MATCH
struct StepPlan {
  StepLaunch at[STAGE_COUNT];
  // the PmStep fields that must agree with the forms
  uint32_t nhelp, nsplit, qw, np_live, cblk, no_guess;
  uint32_t help_spoil;   // PmStep::help_spoil ("step_help_spoil"; k_step only)
  bool qset;   // k_match_resolve_s expands the query sets (PmStep::qset, [nsub][qw]) and the answer reads them
};
// The one selection of a step's kernels, grids and fields: pure (no HIP call, environment or state).
StepPlan step_plan(const StepShape& s, const StepOpts& O);
// Issues one launch of a plan (S as the plan says: pmh::step_chain).
void step_launch(hipStream_t st, const PmStep& S, const StepPlan& plan, int stage, PmEvents ev = {});
// whether step_launch takes the packed instance at `stage`: the pair answer (k_answer_p5 / k_answer_p) of a
// step whose server has the packed row image (PmStep::dbp); counted in "host_answer_packed"
inline bool step_answer_packed(const PmStep& S, const StepPlan& plan, int stage) {
  const int form = plan.at[stage].form;
  return stage == STAGE_ANSWER && (form == FORM_ANSWER_P5 || form == FORM_ANSWER_P) && S.dbp != nullptr;
}
uint32_t step_max_sub_per_part();
uint32_t step_max_ss();
uint32_t step_max_e();
// The client role of a two-party round (pm_batchpir_client_begin / _finish), over a step whose hint search
// and resolution have run (S.res).  k_client_sets: sub-query s's answer mode into modes[s] and, where it
// gathers rows, its query set as u32 into sets[s][0 .. qw) (qw a multiple of 4, zero past SetSize).
// k_client_finish: the answer's epilogue with sub-query s's gathered row read from answers[map[s]]
// (E words each; map[s] = ~0u: no set was sent).  Shapes up to client_max_ss() / client_max_e().
void client_sets(hipStream_t st, const PmStep& S, uint32_t* sets, uint32_t* modes, uint32_t qw);
void client_finish(hipStream_t st, const PmStep& S, const uint64_t* answers, const uint32_t* map);
bool client_mode_sends(uint32_t mode);   // a mode word of k_client_sets whose sub-query sends its set
bool client_mode_reads(uint32_t mode);   // ... and whose answer row k_client_finish reads (not a dummy's)
uint32_t client_max_ss();
uint32_t client_max_e();
void server_answer(hipStream_t st, const PmPart* dpart, const uint32_t* offs, uint32_t nq,
                   uint32_t SS, const uint64_t* db, uint32_t E, uint64_t* out);
// k_server_answer_parts: set s (offs + s * stride) over partition qpart[s] of sp.  dbp: the packed row image
// (pk_nseg / pk_cseg as PmStep's), gathered instead of db when not null.
void server_answer_parts(hipStream_t st, const PmSrvPart* sp, const uint32_t* qpart, const uint32_t* offs,
                         uint32_t nq, uint32_t stride, const uint64_t* db, const uint64_t* dbp, uint32_t pk_nseg,
                         uint32_t pk_cseg, uint32_t E, uint64_t* out);
void l2_rows(hipStream_t st, const float* rows, uint64_t row_stride_floats, uint64_t nrows,
             const uint32_t* row_ids, const float* q, uint32_t dim, float* out, uint64_t seglen = 0);
void ip_rows(hipStream_t st, const uint32_t* rows, uint64_t nrows, const uint32_t* q, uint32_t dim,
             uint32_t* per_row, uint32_t* sum);
void ip_fill(hipStream_t st, uint32_t* rows, uint64_t N, uint32_t D, uint64_t r0 = 0);   // rows r0 .. r0 + N
// Synthetic DB rows (pm_batchpir_create_synth): dst row i = global row r0 + i,
// word w = sm64(sm64(db_seed + DOM_SYNTH_DB) ^ (r * E + w)).
void db_synth(hipStream_t st, uint64_t* dst, uint64_t r0, uint64_t rows, uint32_t E, uint64_t db_seed);
// out[i] = {E words at src[i] (or zeros when null), success flag}, src in pinned host memory
void gather_rows(hipStream_t st, const uint64_t* const* src, uint64_t n, uint32_t E, uint64_t* out);
// ---- sharded private search (pm_shard.hip) ----
// Synthetic graph DB rows (graph_synth_elem): dst row i = global vertex r0 + i,
// E = (dim + m) / 2 words per row.
void graph_synth(hipStream_t st, uint64_t* dst, uint64_t r0, uint64_t rows, uint64_t n, uint32_t dim, uint32_t m,
                 uint64_t seed);
// out[i*dim + j] = vector of vertex ids[i] (the start set, GetStartVertex)
void graph_synth_vecs(hipStream_t st, const uint64_t* ids, uint64_t nids, uint32_t dim, uint64_t seed, float* out);
// Per-id records of a shared step for the shards' combine.  Record r (session
// s = r / npos, position r % npos of its GetVertexInfo batch) = the W - 1 row
// words [w0, w0 + W - 1) of its answer (the neighbour list) and one word
// {dist f32 bits | ok << 32}; map[r] = the answering sub-query of the step
// (a DUP followed to its source) or < 0 (no local answer: zeros).  Also
// st2[j] = {status, ref} of every sub-query j < nsub (the host's mirrors), and
// the error word rec[nrec * W] = errw (0, or 1 from a failed rank: group_exchange).
void pack_records(hipStream_t st, const int32_t* map, uint32_t nrec, const PmOutHdr* hdr, const uint64_t* rows,
                  uint32_t E, uint32_t w0, uint32_t W, uint64_t* rec, uint32_t nsub, uint32_t* st2, uint64_t errw);
// Modelled peers (a shard layout wider than the job): records with map[r] ==
// -2 are those another shard of the layout answers; they are filled from the
// synthetic graph's spec, the distance to session r / npos's query (qbuf) in
// the reference's L2 order (l2_distance_amd64.s:4-36).
void synth_records(hipStream_t st, const int32_t* map, const uint64_t* ids, uint32_t nrec, uint32_t npos,
                   const float* qbuf, uint32_t dim, uint32_t m, uint64_t n, uint64_t seed, uint32_t w0, uint32_t W,
                   uint64_t* rec);
void prf_batch(hipStream_t st, const uint32_t* rk, const uint64_t* tags, const uint64_t* xs,
               uint64_t n, uint64_t* out);
// the device-resident team round (pm_drl.hip): one 64-lane workgroup per session
void team_round(hipStream_t st, const DrlArgs& A, PmEvents ev = {});
uint32_t team_round_lds(uint32_t kcap, uint32_t n, uint32_t m);   // bytes of dynamic LDS
constexpr uint32_t kDrlMaxKcap = 4096, kDrlMaxN = 256, kDrlMaxNM = 8192, kDrlMaxParallel = 8;
// the batched non-private search (pm_knnb.hip): one 256-thread workgroup per
// query.  knn_batch_kcap: known-set capacity, the next power of two >=
// parallel (1 + max_step m) (0: beyond any LDS); knn_batch_lds: bytes of
// dynamic LDS; knn_batch_ok: whether the shape runs on the device.
constexpr uint32_t kKnbMaxBatch = 256, kKnbMaxM = 64, kKnbMaxLds = 160 * 1024 - 512;
uint32_t knn_batch_kcap(uint64_t parallel, uint64_t max_step, uint64_t m);
uint64_t knn_batch_lds(uint32_t kcap, uint32_t dim, uint32_t nb, uint32_t ns);
bool knn_batch_ok(uint64_t dim, uint64_t m, uint64_t ns, uint64_t max_step, uint64_t parallel);
void knn_batch(hipStream_t st, const KnbArgs& A);
// graph construction and ground truth (pm_graph.hip).  One entry per stage; each picks its kernel's
// instantiation from the row width and top, the keys kept per query row (knn_top() or knn_top_k128()).
inline unsigned gcdiv(uint64_t a, uint64_t b) { return (unsigned)((a + b - 1) / b); }
// the grid of a kernel that loops over gridDim.x: at most 2^20 blocks
inline unsigned gclamp(uint64_t blocks) { return (unsigned)(blocks < (1u << 20) ? blocks : (1u << 20)); }
uint32_t knn_pad_dim(uint32_t dim);        // bf16 row width of rows held whole, 128 or 192 (0: too wide)
uint32_t knn_pad_dim_wide(uint32_t dim);   // ... of any row: the next multiple of 64 (0: dim 0 or above 1,024)
bool knn_wide(uint32_t width);             // a dim or padded width above knn_pad_dim's: the chunked / one-row-in-LDS kernels
uint32_t knn_top();                        // 64
uint32_t knn_top_k128();                   // 128
uint32_t prune_max_list();
uint32_t prune_max_dim();
uint32_t prune_max_m();
void to_bf16(hipStream_t st, const float* rows, uint64_t n, uint32_t dim, uint32_t dp, void* out, float* norms);
void knn_prefilter(hipStream_t st, const void* X, const float* xn, uint64_t N, const void* Q, const float* qn,
                   uint64_t M, uint32_t dp, uint32_t* out, uint32_t* out_hi = nullptr);
void knn_rerank(hipStream_t st, const float* X, uint64_t N, uint32_t dim, const float* Q, uint64_t M,
                const uint32_t* cand, uint32_t K, bool self_base, uint32_t* out, float* dist, uint32_t* len);
// the exact variants (pm_knn_exact, _wide, _k128): split rows hi + lo with f32 norms and the largest
// norm's bits; the three-product prefilter at any padded width (128, 192, or a multiple of 64 up to
// 1,024) with out / out_hi [M][top] and each row's last prefilter distance tau; the re-rank with the
// certificate (uncertified rows appended to list, counted in *nlist); the brute-force fallback of the
// listed rows at any dim up to 1,024; and the relative part of the certificate's eps at width dp
void to_bf16x2(hipStream_t st, const float* rows, uint64_t n, uint32_t dim, uint32_t dp, void* hi, void* lo,
               float* norms, uint32_t* maxnorm);
void knn_prefilter_x3(hipStream_t st, const void* Xh, const void* Xl, const float* xn, uint64_t N, const void* Qh,
                      const void* Ql, const float* qn, uint64_t M, uint32_t dp, uint32_t top, uint32_t* out,
                      float* tau, uint32_t* out_hi = nullptr);
float knn_cert_rel(uint32_t dp);
void knn_rerank_cert(hipStream_t st, const float* X, uint64_t N, uint32_t dim, const float* Q, uint64_t M,
                     const uint32_t* cand, uint32_t K, bool self_base, uint32_t* out, float* dist, uint32_t* len,
                     const float* qn, const float* tau, const uint32_t* maxnorm, uint32_t dp, uint32_t top,
                     uint64_t* list, uint64_t* nlist, float* eps_out = nullptr);
void knn_brute(hipStream_t st, const float* X, uint64_t N, uint32_t dim, uint32_t top, const float* Q,
               const uint64_t* list, uint64_t nlist, uint32_t K, bool self_base, uint32_t* out, float* dist,
               uint32_t* len);
// wide: the caller is an entry point for rows up to 1,024; its rows above knn_pad_dim's take the form
// with one row in LDS, every other call the form with the accepted rows in LDS (dim <= prune_max_dim())
void prune(hipStream_t st, const float* X, uint32_t dim, bool wide, const uint32_t* verts, uint64_t nverts,
           const uint64_t* offs, uint64_t stride, const uint32_t* lens, const uint32_t* ids, uint32_t m,
           float alpha, uint32_t* out, uint32_t* out_len, uint32_t* err, const uint32_t* sorted_pos = nullptr,
           const float* dist_g = nullptr);
// L2Dist of every candidate of the listed vertices (hub lists above prune_max_list())
void cand_dist(hipStream_t st, const float* X, uint32_t dim, const uint32_t* verts, uint64_t nverts,
               const uint64_t* offs, const uint32_t* lens, const uint32_t* ids, float* dist_g);
// uint8 rows on the int8 matrix cores (pm_graph_u8.hip; pm_knn_u8, pm_build_graph_u8): u8_bias writes
// n rows of dp bytes (x ^ 0x80, 0 padded; dp = knn_u8_pad_dim(dim): the next multiple of 64, 0 above
// knn_u8_max_dim()) and the rows' int32 constants; knn_i8 the first K (K <= 128) of every query
// row's (integer distance, id) ranking, out / dist [M][K] and len [M] as knn_rerank's.
uint32_t knn_u8_max_dim();
uint32_t knn_u8_pad_dim(uint32_t dim);
void u8_bias(hipStream_t st, const uint8_t* rows, uint64_t n, uint32_t dim, uint32_t dp, void* out, int32_t* cst);
void u8_to_f32(hipStream_t st, const uint8_t* rows, uint64_t count, float* out);
void knn_i8(hipStream_t st, const void* X, const int32_t* xc, uint64_t N, const void* Q, const int32_t* qc, uint64_t M,
            uint32_t dp, uint32_t K, bool self_base, uint32_t* out, float* dist, uint32_t* len);
// k-means and the cluster search (pm_cluster.hip; pm_kmeans, pm_cluster_*).
// cluster_sort: order [n] = the ids sorted by (label, id) and offs [nc + 1] = the first position of every
// label, through keys (label << idbits | id) sorted into keys_out (both [n]); temp of cluster_sort_temp(n, nc)
// bytes.  kmeans_update: centroid c = the f64 mean of rows order[offs[c] .. offs[c + 1]) in the order of
// DESIGN.md §10.5, unchanged for an empty cluster.  kmeans_moved: *count += the rows with cur != prev.
// cluster_gather: out row r = rows[order[r]].  cluster_scan: list e [K] = the K smallest (L2Dist(row r,
// query work[e].q) bits << 32 | order[r]) keys over the rows [r0, r1) of S, ascending, kNoKey padded;
// cluster_merge: query q's result = the K smallest keys of lists woff[q] .. woff[q + 1), out / dist [nq][K]
// and len [nq] as knn_rerank's.
struct ScanWork {
  uint64_t r0, r1;   // rows of the cluster-ordered copy, r0 < r1
  uint32_t q, pad;   // the query row
};
constexpr uint32_t kKmeansPartials = 16;   // partial sums per coordinate (part of pm_kmeans' contract)
size_t cluster_sort_temp(uint64_t n, uint64_t nc);
hipError_t cluster_sort(hipStream_t st, void* temp, size_t temp_bytes, const uint32_t* labels, uint64_t n, uint64_t nc,
                        uint64_t* keys, uint64_t* keys_out, uint32_t* order, uint64_t* offs);
void kmeans_update(hipStream_t st, const float* rows, uint32_t dim, const uint32_t* order, const uint64_t* offs,
                   uint64_t nc, float* centroids);
void kmeans_moved(hipStream_t st, const uint32_t* cur, const uint32_t* prev, uint64_t n, uint64_t* count);
void cluster_gather(hipStream_t st, const float* rows, uint64_t n, uint32_t dim, const uint32_t* order, float* out);
void cluster_scan(hipStream_t st, const float* S, const uint32_t* order, uint32_t dim, const float* Q,
                  const ScanWork* work, uint64_t nwork, uint32_t K, uint64_t* lists);
void cluster_merge(hipStream_t st, const uint64_t* lists, const uint64_t* woff, uint64_t nq, uint32_t K, uint32_t* out,
                   float* dist, uint32_t* len);
}  // namespace pmk
