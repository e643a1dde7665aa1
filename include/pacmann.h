/*
 * pacmann.h — C ABI of libpacmann.so, the MI355X (gfx950) implementation of
 * Pacmann's two data-parallel inner loops (wuwuz/Pacmann):
 *
 *   1. PianoPIR: AES-128-MMO PRF set expansion + 64-bit XOR database fold
 *      (client hint preprocessing, server answer, online hint search and
 *      refresh, 16-way batch PIR), bit-exact with the pianopir Go code + aes_amd64.s.
 *   2. graphann: batched L2 / uint32 inner-product distance evaluation that
 *      drives the degree-m beam search, bit-exact with l2_distance_amd64.s.
 *
 * The entry points replace the reference's Go package surfaces at method /
 * batch granularity (never per PRF or per 640-B XOR: a launch per leaf would
 * cost more than the Go assembly it replaces).  Each function cites the
 * reference interface it stands in for.  All pointers are HOST pointers;
 * device memory is owned by the library behind opaque handles.  Input host
 * buffers are copied and never retained; output buffers are caller-allocated.
 * Every function returns 0 on success or a negative PM_E* code; the message
 * is in pm_last_error() (thread-local).  The library never aborts the process
 * (the reference's log.Fatalf paths return PM_EINVAL instead).
 *
 * Threading: one handle per host thread; handles are not thread-safe (the
 * reference's PianoPIRClient is not either, pir.go:91-121).
 */
#ifndef PACMANN_H
#define PACMANN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PM_OK 0
#define PM_EINVAL -1   /* bad argument / reference log.Fatalf condition   */
#define PM_EHIP -2     /* HIP runtime error                              */
#define PM_ENOMEM -3   /* device allocation failed                       */
#define PM_ETIMEDOUT -4 /* a bounded wait expired (RCCL peer never joined) */

/* Per-sub-query status codes (pianopir/pir.go:354-471 error returns). */
#define PM_Q_OK 0          /* answered through PIR                             */
#define PM_Q_EBUDGET 1     /* "exceed the maximum number of queries" :386-391  */
#define PM_Q_ECHUNK 2      /* "too many queries in chunk" :396-400             */
#define PM_Q_ENOHIT 3      /* "no hit hint in the primary hint table" :416-419 */
#define PM_Q_ERANGE 4      /* idx out of range (:373-378 log.Fatalf)           */

typedef struct pm_ctx pm_ctx;
typedef struct pm_pir pm_pir;           /* PianoPIR             (pir.go:473-477)       */
typedef struct pm_batchpir pm_batchpir; /* SimpleBatchPianoPIR  (batch-pir.go:40-53)   */
typedef struct pm_graph pm_graph;       /* GraphANNFrontend + PIRGraphInfo / BasicGraphInfo */

/* ---- context ----------------------------------------------------------- */
int         pm_ctx_create(int device, pm_ctx** out);
void        pm_ctx_destroy(pm_ctx* ctx);
const char* pm_last_error(void);
int         pm_ctx_sync(pm_ctx* ctx);
/* Free and total device memory of the context's GPU (bytes; sizing how many
 * client sessions a GPU holds next to its DB). */
int         pm_ctx_mem_info(pm_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes);
/* Per-kernel timing.  Level 1: HIP events around the preprocessing and leaf
 * kernels on the stream they run on ("prep_offsets", "prep_fold",
 * "prep_repl", "l2_rows", "ip_scan", "prf", server "answer" and
 * "server_answer").  Level 2 also
 * times the kernels of every online step ("step", "hint_match", "resolve",
 * "gather", "answer") with events carried in their own dispatch packets
 * (hipExtLaunchKernelGGL); steps are not synchronised for it (the events are
 * read by pm_timing_get).  Level 3 is level 2 with the kernels of a lock-step
 * team's shared steps timed on every 7th step of its stream only (the serving
 * bench: a sample, at a fraction of the events' cost).  Host wall-clock
 * accumulators are always on: "host_step_launch", "host_step_wait",
 * "host_step_post", "host_batch_query", "host_gvi_parse", "host_search_knn",
 * "host_knn_init", "host_knn_batch", "host_knn_update", "host_knn_final";
 * "host_gvi_group" (the wall time of pm_graph_group_get_vertex_info, one entry
 * per call that fetched anything) and "host_gvi_group_steps" (the shared steps
 * those calls launched: a count, total_ms 0), both on sessions[0]'s context.
 * So are the step-form counters, one launch count per kernel form as the
 * step's plan launched it (total_ms 0 unless noted), on the
 * context whose stream ran the step: "host_path_match", "host_path_match_part",
 * "host_path_match_part8" (k_match, k_match_part, k_match_part8);
 * "host_path_step" (the fused k_step<W>; total_ms = the sum of its gather
 * helpers per sub-query, a count); "host_path_resolve_lds",
 * "host_path_resolve_g" (k_resolve<true>, <false>); "host_path_mr_s2",
 * "host_path_mr_s4", "host_path_mr_general" (k_match_resolve_s<2,256>,
 * <4,256>, k_match_resolve); "host_path_gather" (k_gather<W>);
 * "host_path_answer_p5", "host_path_answer_p", "host_path_answer_s",
 * "host_path_answer_g" (k_answer_p5, k_answer_p, k_answer_s<W,NT>,
 * k_answer<W>).  step_plan (pm_query.hip) is the single place that selects
 * them (pm_step_plan shows its answer; DESIGN.md §5 lists the shapes). */
int pm_timing_enable(pm_ctx* ctx, int level);
/* "rccl_timeout_s": the bound (seconds) on RCCL communicator creation and
 * its probe (pm_rccl_create / pm_rccl_probe); "verify_records" (sharded loop):
 * check every value-th shared step's records on the host.
 * Process-wide choice among equivalent kernel paths (no reference counterpart:
 * the same results by every path; tests drive each one).  "match_part": the
 * hint search per (partition, block) instead of per (sub-query, block), -1
 * automatic / 0 / 1; "match_part8": its one-wave-per-block form where PH % 8 ==
 * 0, 0 / 1; "match_resolve": k_match_resolve* for search-sized steps, 0 / 1 /
 * 2 (the general form).  -2 restores the environment's choice (PM_MATCH_PART,
 * PM_MATCH_PART8, PM_MATCH_RESOLVE).  "step_help": k_step's gather helpers per
 * sub-query, 0..3 (-2: PM_STEP_HELP, default 3), still capped by the launch's
 * workgroup budget (pm_step_plan's nhelp).  "step_help_spoil" (tests): a mask of
 * helpers 1..3 (bits 0..2) that hand over their partial with a guess no answer
 * accepts, so the answers refuse the helpers and gather again; no form, grid or
 * result changes (-2 / 0: off); other values of either are PM_EINVAL.  "aes_bs": the preprocessing's PRF tables
 * by the bitsliced VALU AES (1) or the T-table AES (0, default; -1: PM_AES_BS).
 * "fold_rot": the hint fold of ChunkSize 512 / 1,024 partitions by the
 * bank-rotated kernel over a fold image of the DB (1) or by the pipelined fold
 * over the rows themselves (0), which is also what runs when the image does
 * not fit in device memory; -1: PM_FOLD_ROT (default on); any other value is
 * PM_EINVAL.  Read when a server or client is created, never later: each keeps
 * the form it was created with for all its preprocessings, a client of a server
 * without an image goes without one, and clients preprocessed as one group
 * must agree (PM_EINVAL otherwise).
 * "fold_pack": whether a graph DB (pm_graph_*) whose coordinates all have zero
 * low halves (f32 holding small integers, e.g. SIFT's bytes; detected once,
 * when the server packs its DB) gets a packed fold image without those halves
 * (1, at ChunkSize 512 and dim % 16 == 0) or the plain image (0); -1:
 * PM_FOLD_PACK (default on); any other value is PM_EINVAL.  Read when a server
 * is created; its clients and sessions share the image and the decision.
 * "host_fold_rot512p" counts the folds over a packed image, "host_fold_rot512"
 * those over a plain one.
 * "fold_bits": whether such a DB whose coordinates also have a clear sign and
 * equal exponent bits 6..3 (f32 holding 0..255), or whose neighbour ids are
 * below 2^20, gets a bit-packed fold image of 12-bit coordinate and / or 20-bit
 * id fields where that has fewer 32-B slices than the packed image (1) or stays
 * with the packed image (0); -1: PM_FOLD_BITS (default on); any other value is
 * PM_EINVAL.  Read with "fold_pack", which must be on.  "host_fold_rot512q"
 * counts the folds over a bit-packed image; its total adds up their slices.
 * "answer_pack": whether such a graph DB (zero low halves in every coordinate
 * word, E % 4 == 0, E <= 256 words, dim % 8 == 0) also gets a packed row image
 * (rows of 2 dim + 4 (2E - dim) bytes: the coordinates' high halves, then the
 * other words whole) which the pair answer kernels of shared steps gather
 * instead of the DB's rows (1), or not (0); -1: PM_ANSWER_PACK (default on); any
 * other value is PM_EINVAL.  Read when a server is created; its clients and
 * sessions share the image and the decision.  "host_answer_packed" counts the
 * "host_path_answer_p5" / "host_path_answer_p" launches that gathered it.
 * "device_loop": the batched serving loop on the device (1 / 0; -1 automatic).
 * "fault_drl_query" (tests): the device loop fails before queueing query
 * `value` (-1 off); its sessions are then unusable (every later call on them
 * returns PM_EINVAL: their host counters no longer match the device state).
 * "stream_upload_only" (probes): 1 = pm_batchpir_prep_stream_rows stages and
 * uploads its sub-windows without launching its kernels (0 default).
 * PM_EINVAL for an unknown name. */
int pm_set_option(const char* name, int value);
/* Which kernels an online step of a given shape launches: the answer of the one
 * selector every step asks (step_plan, pm_query.hip), under the current
 * pm_set_option / environment choices.  Host arithmetic only: no context, no
 * device, nothing launched.  kind: 0 an engine's own step (pm_pir_query,
 * pm_batchpir_query*), 1 a group's shared step (pm_batchpir_group_query, the
 * host serving loops), 2 a shared step of the device loop; where the step's
 * descriptor lives follows from it and the sizes.  np: partitions of the step
 * (clients x partitions for a shared one), nsub: its sub-queries, np_live:
 * partitions with at least one, max_per_part: the most sub-queries of one
 * partition; maxPH / maxSS: the largest PrimaryHintNum / SetSize, E: entry
 * words, ph8: every PrimaryHintNum is a multiple of 8; no_fuse: PM_NO_FUSE or
 * PM_DEBUG_SYNC, no_split: PM_NO_SPLIT, no_guess: PM_NO_GUESS of the context.
 * Out, per launch in the order fused step, match + resolve, hint search,
 * resolve, gather, answer: the "host_path_*" counter the launch counts in
 * (pm_timing_enable; NULL: not launched), its grid and block; then the step
 * fields that go with the forms (nhelp: k_step's gather helpers per sub-query,
 * nsplit: gather ranges, qw / qset: pre-expanded query sets).  PM_EINVAL for a
 * NULL argument, an unknown kind or an empty step. */
typedef struct pm_step_shape {
  uint32_t kind, np, nsub, np_live, max_per_part, maxPH, maxSS, E, ph8, no_fuse, no_split, no_guess;
} pm_step_shape;
typedef struct pm_step_forms {
  const char* counter[6];
  uint32_t grid_x[6], grid_y[6], block[6];
  uint32_t nhelp, nsplit, qw, np_live, cblk, no_guess, qset, args_valid;
} pm_step_forms;
int pm_step_plan(const pm_step_shape* shape, pm_step_forms* out);
/* The index map of the fold image the server builds (k_fold_image), as the
 * kernel itself evaluates it.  Host arithmetic only.  A partition of ChunkSize
 * cs (512 / 1,024) and SetSize ss with E-word entries has an image of *nitems
 * 16-B items; for items [x0, x0 + n): row[i] the partition row the item is
 * taken from (rows past the partition's end are stored as zero), word[i] the
 * first 32-bit word of that row it holds, is_packed[i] 0 if it holds four whole
 * words, 1 if it holds the high halves of eight as consecutive half-words.
 * packed != 0: the packed image of entries whose first dim 32-bit words are
 * coordinates, *npk its packed slices; PM_EINVAL if such entries have none
 * (dim % 16 != 0, coordinates beyond the folded words, cs != 512). */
int pm_fold_image_map(uint32_t cs, uint32_t ss, uint32_t E, uint32_t dim, int packed, uint64_t x0, uint64_t n,
                      uint64_t* row, uint32_t* word, uint8_t* is_packed, uint64_t* nitems, uint32_t* npk);
int pm_timing_reset(pm_ctx* ctx);
/* Diagnostics: append one line "kernel,start_us,end_us,ctx" per timed launch
 * of ctx (level >= 2 timing) to the file at `path`, on one time axis for every
 * context of the process (the GPU timeline of a serving run). */
int pm_timing_timeline(pm_ctx* ctx, const char* path);
int pm_timing_get(pm_ctx* ctx, const char* kernel, uint64_t* launches, double* total_ms,
                  double* alg_bytes);

/* ---- leaf primitives, batched ----------------------------------------- */
/* expandKeyAsm (pianopir/aes_amd64.s:87-126): FIPS-197 AES-128 key schedule. */
int pm_expand_key(const uint8_t key[16], uint32_t round_keys[44]);
/* PRFEvalWithLongKeyAndTag (pianopir/util.go:157-165) over n (tag, x) pairs on
 * the GPU: out[i] = low64_LE(AES_k(B) ^ B), B = LE64((tag<<35)+x) || 0^8. */
int pm_prf_batch(pm_ctx* ctx, const uint32_t round_keys[44], const uint64_t* tags,
                 const uint64_t* xs, uint64_t n, uint64_t* out);
/* L2Dist (graphann/build_graph.go:119-127 -> l2_distance_amd64.s:4-36) of one
 * query against nrows rows (row-major nrows x dim), bit-exact. */
int pm_l2_batch(pm_ctx* ctx, const float* query, const float* rows, uint64_t nrows,
                uint64_t dim, float* out);
/* InnerProduct (l2_distance_amd64.s:39-68) of one query against nrows rows:
 * per-row uint32 dot products mod 2^32 (per_row may be NULL) and their
 * wrapping sum. */
int pm_ip_batch(pm_ctx* ctx, const uint32_t* query, const uint32_t* rows, uint64_t nrows,
                uint64_t dim, uint32_t* per_row, uint32_t* sum);
/* TestInnerProduct scan (graphann/graphann_test.go:249-283) fully on device:
 * fills vectors[i*D+j] = i+j in HBM, query[j] = j, then sums the N row dot
 * products mod 2^32.  scan_ms = device time of the scan kernel alone. */
int pm_ip_bench(pm_ctx* ctx, uint64_t N, uint64_t D, uint32_t* sum, double* scan_ms);
/* The same scan over rows [r0, r0 + rows) of the N-row fill: one GPU's shard
 * of the row-sharded scan (scans shard by rows, the mod-2^32
 * partial sums add up to TestInnerProduct's sum).  r0 + rows <= N. */
int pm_ip_bench_shard(pm_ctx* ctx, uint64_t N, uint64_t D, uint64_t r0, uint64_t rows, uint32_t* sum,
                      double* scan_ms);

/* ---- PianoPIR (pianopir/pir.go) --------------------------------------- */
typedef struct {
  uint64_t DBEntryByteNum, DBEntrySize, DBSize, ChunkSize, SetSize, ThreadNum, FailureProbLog2;
  uint64_t MaxQueryNum, PrimaryHintNum, MaxQueryPerChunk, FinishedQueryNum;
} pm_pir_config;

/* NewPianoPIR(DBSize, DBEntryByteNum, rawDB, FailureProbLog2) (pir.go:479-514).
 * seed drives the key / replacement / dummy streams that the
 * reference draws from time-seeded math/rand (pir.go:132,208,305,366). */
int    pm_pir_create(pm_ctx* ctx, uint64_t DBSize, uint64_t DBEntryByteNum, const uint64_t* rawDB,
                     uint64_t FailureProbLog2, uint64_t seed, pm_pir** out);
void   pm_pir_destroy(pm_pir* h);
int    pm_pir_preprocessing(pm_pir* h);          /* PianoPIR.Preprocessing      pir.go:516-518 */
int    pm_pir_dummy_preprocessing(pm_pir* h);    /* PianoPIR.DummyPreprocessing pir.go:520-523 */
/* PianoPIR.Query(idx, realQuery) (pir.go:525-533); *status = PM_Q_* */
int    pm_pir_query(pm_pir* h, uint64_t idx, int real, uint64_t* out, int* status);
int    pm_pir_config_get(pm_pir* h, pm_pir_config* cfg);   /* PianoPIR.Config  pir.go:546-548 */
double pm_pir_local_storage(pm_pir* h);                    /* LocalStorageSize pir.go:178-190 */
double pm_pir_comm_per_query(pm_pir* h);                   /* CommCostPerQuery pir.go:539-544 */
/* PianoPIRServer.PrivateQuery (pir.go:65-88), batched: nq offset sets of
 * SetSize uint32 each -> nq entries of DBEntrySize words. */
int    pm_pir_server_answer(pm_pir* h, const uint32_t* offsets, uint64_t nq, uint64_t* out);

/* ---- SimpleBatchPianoPIR (pianopir/batch-pir.go) ---------------------- */
typedef struct {
  uint64_t DBEntryByteNum, DBEntrySize, DBSize, BatchSize, PartitionNum, PartitionSize,
           ThreadNum, FailureProbLog2;
  uint64_t FinishedBatchNum, QueriesMadeInPartition, SupportBatchNum, PrepCount;
  double   LocalStorage, PreprocessingTime, CommOnline, CommOffline;
} pm_batchpir_stats;

/* NewSimpleBatchPianoPIR (batch-pir.go:55-93) */
int  pm_batchpir_create(pm_ctx* ctx, uint64_t DBSize, uint64_t DBEntryByteNum, uint64_t BatchSize,
                        const uint64_t* rawDB, uint64_t FailureProbLog2, uint64_t seed,
                        pm_batchpir** out);
/* One shard of the same batch PIR for multi-GPU use: this
 * handle keeps the DB slice, keys and hint state of the partitions p with
 * p % nshards == shard only (rawDB is still the whole DB; only those rows are
 * uploaded).  Bucketing, dummies, drops, counters and the re-preprocessing
 * trigger are the global ones, so every shard, fed the same batches, makes the
 * same decisions; pm_batchpir_query(_ok) fills the entries of its own
 * partitions and leaves the others zero (ok = 0).  Summing the entries (and
 * OR-ing ok) over all shards gives the unsharded answer bit for bit (keys
 * derive from the global partition index). */
int  pm_batchpir_create_shard(pm_ctx* ctx, uint64_t DBSize, uint64_t DBEntryByteNum, uint64_t BatchSize,
                              const uint64_t* rawDB, uint64_t FailureProbLog2, uint64_t seed,
                              uint32_t shard, uint32_t nshards, pm_batchpir** out);
/* The same shard over a synthetic DB generated on the device (BIGANN-scale
 * benchmarks, BASELINE.json configs[3]/[4]: tens of GB never cross PCIe).  It
 * replaces the reference's in-process random DB of TestBatchPIRPerf
 * (pir_test.go:204-275).  Word w of global row r is
 *   sm64(sm64(db_seed + 9) ^ (r * DBEntrySize + w)),
 * sm64 = the splitmix64 finalizer of (x + 0x9e3779b97f4a7c15),
 * so a caller can recompute any row to check an answer. */
int  pm_batchpir_create_synth(pm_ctx* ctx, uint64_t DBSize, uint64_t DBEntryByteNum, uint64_t BatchSize,
                              uint64_t FailureProbLog2, uint64_t seed, uint64_t db_seed, uint32_t shard,
                              uint32_t nshards, pm_batchpir** out);
/* Another client of the same server (multi-session serving, SURVEY.md §8f
 * rank 2): a new SimpleBatchPianoPIR client (own keys from `seed`, own hint
 * state, counters and local cache) whose server side reads the DB rows of
 * `server` in place (one device copy of the DB for all its clients; the
 * reference's server likewise keeps one rawDB alias, pir.go:34-39).  Same
 * DBSize, entry size, BatchSize, FailureProbLog2 and shard as `server`; same
 * device as `ctx`.  The DB stays alive while any client holds it. */
int  pm_batchpir_create_client(pm_ctx* ctx, pm_batchpir* server, uint64_t seed, pm_batchpir** out);
void pm_batchpir_destroy(pm_batchpir* h);
int  pm_batchpir_preprocessing(pm_batchpir* h);         /* batch-pir.go:119-155 */
int  pm_batchpir_dummy_preprocessing(pm_batchpir* h);   /* batch-pir.go:157-166 */
/* Query (batch-pir.go:170-248): out = n x DBEntrySize words; dropped or failed
 * ids get an all-zero entry exactly like the reference. */
int  pm_batchpir_query(pm_batchpir* h, const uint64_t* ids, uint64_t n, uint64_t* out);
/* The same query with a per-id success mask: ok[i] = 1 when entry i is the
 * answer of a successful sub-query (or its local-cache copy), 0 when the id
 * was dropped by the bucketing (batch-pir.go:195-200) or its sub-query failed
 * (the error batch-pir.go:205 swallows); those entries are zero. */
int  pm_batchpir_query_ok(pm_batchpir* h, const uint64_t* ids, uint64_t n, uint64_t* out, uint8_t* ok);
/* The same query with the responses left in DEVICE memory, for an in-place
 * collective over the shards (the multi-GPU combine, SURVEY.md §8e;
 * replaces the host round trip of Query's [][]uint64 result, batch-pir.go:
 * 216-236): dev_out is a device pointer on this handle's GPU of
 * n x (DBEntrySize + 1) uint64 words; row i holds id i's entry and, in word
 * DBEntrySize, 1 when it is a successful answer (pm_batchpir_query_ok's flag)
 * or 0 (entry zero).  Entries are copied HBM to HBM from the partitions'
 * local caches.  stream: a HIP stream (hipStream_t) of the consumer, made to
 * wait for the rows without a host synchronisation; NULL: the rows are written
 * when the call returns. */
int  pm_batchpir_query_dev(pm_batchpir* h, const uint64_t* ids, uint64_t n, uint64_t* dev_out, void* stream);
int  pm_batchpir_stats_get(pm_batchpir* h, pm_batchpir_stats* s);
/* Many clients of one server answered together (batched serving, SURVEY.md
 * §8f rank 2): every pm_batchpir_group_query call makes, for each client s,
 * exactly the SimpleBatchPianoPIR.Query (batch-pir.go:170-248) call of its batch
 * ids[s*n .. s*n+n), with all clients' sub-queries in ONE shared step over
 * S x 16 partitions (on clients[0]'s stream).  out: S x n x DBEntrySize words,
 * ok (nullable): S x n success flags, as pm_batchpir_query_ok.  Clients: the
 * server and/or pm_batchpir_create_client handles of one server. */
typedef struct pm_batchpir_group pm_batchpir_group;
int  pm_batchpir_group_create(pm_batchpir** clients, uint32_t S, pm_batchpir_group** out);
int  pm_batchpir_group_query(pm_batchpir_group* g, const uint64_t* ids, uint64_t n, uint64_t* out, uint8_t* ok);
/* SimpleBatchPianoPIR.Preprocessing (batch-pir.go:119-155) of every client of
 * the group as ONE launch set on clients[0]'s stream: each partition's clients
 * are folded side by side over the shared DB (the batched serving loop's
 * maintenance).  Every client's state equals its own pm_batchpir_preprocessing. */
int  pm_batchpir_group_preprocessing(pm_batchpir_group* g);
void pm_batchpir_group_destroy(pm_batchpir_group* g);
int  pm_batchpir_subconfig(pm_batchpir* h, uint64_t partition, pm_pir_config* cfg);
/* The server role alone, for clients that keep their keys and hints elsewhere
 * (DESIGN.md §6.6): the batch PIR's partitions are PartitionNum servers
 * (batch-pir.go:62-85), and row s of out is PianoPIRServer.PrivateQuery
 * (pir.go:65-88) of the offset set offsets[s*stride .. s*stride + SetSize(P))
 * over partition P = parts[s]: the XOR over chunks i < SetSize(P) of P's row
 * i*ChunkSize(P) + offsets[i], a term with i*ChunkSize + offsets[i] >=
 * DBSize(P) skipped (pir.go:75-77), words [DBEntrySize & ~3, DBEntrySize) zero
 * (EntryXor).  pm_batchpir_subconfig gives each partition's DBSize, ChunkSize
 * and SetSize; offsets past SetSize(P) inside the stride are ignored.
 * The call reads the handle's DB only (a graph server's packed row image where
 * it has one: "host_server_answer_packed" counts those launches) and neither
 * reads nor writes keys, hints, counters, cache or id stream, so it may run
 * between client calls and works on a handle never preprocessed, on a
 * pm_batchpir_create_client handle and on pm_graph_pir(g).  Synchronous; sets
 * go up and answers come down in chunks of 65,536, one "server_answer" launch
 * (timing level 1) each.
 * PM_EINVAL, before any HIP call and with out untouched: a NULL argument;
 * "stride must be >= the largest SetSize" (pm_batchpir_max_set_size);
 * "partition out of range"; "partition not on this shard"; "offset out of
 * range" for one of a set's first SetSize offsets >= ChunkSize (the reference
 * would read past the chunk).  nq == 0 returns 0. */
int  pm_batchpir_server_answer(pm_batchpir* h, const uint32_t* parts /* nq */,
                               const uint32_t* offsets /* nq x stride */, uint64_t stride,
                               uint64_t nq, uint64_t* out /* nq x DBEntrySize */);
uint64_t pm_batchpir_max_set_size(pm_batchpir* h);   /* max SetSize over the handle's partitions; 0 for NULL */
/* The client role alone: one SimpleBatchPianoPIR.Query
 * (batch-pir.go:170-248) cut at the wire.  pm_batchpir_client_begin buckets the
 * ids, runs the step's hint search and resolution (Client.Query up to
 * pir.go:444) and returns, in sub-query order (partition-major, slot order
 * within a partition), one offset set per sub-query that reaches
 * server.PrivateQuery: parts[s] its partition, offsets[s*stride .. +SetSize(P))
 * the set with the programmed point and the replacement substituted
 * (pir.go:430-439; a dummy's random set, :363-371), [SetSize(P), stride) zero;
 * *nq sets in all.  Cached, duplicate, failed and skipped sub-queries send
 * nothing.  The arrays are pm_batchpir_server_answer's input on any handle over
 * the same DB.  pm_batchpir_client_finish takes that call's nq x DBEntrySize
 * answers (a dummy set's row is not read) and does the rest of Query: decode,
 * hint refresh, localCache, the responses (out, ok as pm_batchpir_query_ok),
 * the batch counters and the re-preprocessing trigger, which preprocesses over
 * the handle's own DB as Query does.  Results, counters and exported state
 * are bit-identical to pm_batchpir_query_ok of the same ids.
 * begin opens a split query on the handle and finish closes it; the calls
 * alternate strictly.  While one is open every other client call on the handle
 * (pm_batchpir_query*, a group query it is a member of, begin, the graph calls
 * over pm_graph_pir, pm_batchpir_dummy_preprocessing) fails with PM_EINVAL, "a
 * split query is open", and changes nothing; pm_batchpir_preprocessing is
 * allowed and closes it (pm_batchpir_group_preprocessing of a group with such a
 * member and pm_graph_group_preprocess are refused like the other calls:
 * preprocess the handle itself); pm_batchpir_server_answer is always allowed.  There is
 * NO ABORT: when begin returns, the resolver has already advanced the hints'
 * tags and program points, the histograms and FinishedQueryNum, so the only
 * ways on are finish and a preprocessing.
 * PM_EINVAL before any HIP call and with nothing changed: a NULL argument; an
 * id >= DBSize; stride < pm_batchpir_max_set_size(h); cap <
 * pm_batchpir_client_max_sets(h, n); n / PartitionNum equal to 0 or above the
 * step's sub-queries per partition; finish with no open query or with nq not
 * the value begin returned; a shard handle (nshards > 1); DBEntrySize > 256
 * words or a SetSize > 1,024.  begin also refuses, with "partition at its query
 * budget: preprocess first" and nothing changed, a batch that would take a
 * partition to MaxQueryNum (where Query re-preprocesses mid-batch,
 * pir.go:527-530): preprocess and call begin again; with n / PartitionNum <= 2
 * this cannot occur.  A HIP failure inside begin (PM_EHIP / PM_ENOMEM) is not
 * such a refusal: the buffers are reserved before anything moves, but a failed
 * launch or copy can leave the dummy counters or the hints advanced; preprocess
 * the handle before using it again.  Timing names: "client_sets", "client_finish" (level 1),
 * "host_client_begin", "host_client_finish". */
uint64_t pm_batchpir_client_max_sets(pm_batchpir* h, uint64_t n);   /* PartitionNum * (n / PartitionNum); 0 for NULL */
int  pm_batchpir_client_begin(pm_batchpir* h, const uint64_t* ids, uint64_t n,
                              uint32_t* parts /* cap */, uint32_t* offsets /* cap x stride */,
                              uint64_t stride, uint64_t cap, uint64_t* nq);
int  pm_batchpir_client_finish(pm_batchpir* h, const uint64_t* answers /* nq x DBEntrySize */,
                               uint64_t nq, uint64_t* out /* n x DBEntrySize */,
                               uint8_t* ok /* n, nullable */);
/* A SimpleBatchPianoPIR client with no DB on the device. */
/* The deployment of the two roles above: keys and hints on the client's
 * machine, rows on the server's.  The handle is a client in everything but the
 * DB: every partition's parameters, keys, hint tables, counters, bucketing and
 * localCache, with no rows, no fold image and no packed row image.  Its hints
 * come from streamed preprocessings (below); pm_batchpir_export, _subconfig,
 * _stats_get, _max_set_size, _client_max_sets, _client_begin and _client_finish
 * work as on any client.  Every call that would read the DB fails with
 * PM_EINVAL, "no DB on this handle", before any HIP call and with nothing
 * changed: pm_batchpir_query*, pm_batchpir_preprocessing,
 * pm_batchpir_server_answer, pm_batchpir_server_rows, pm_batchpir_create_client
 * with it as server, pm_batchpir_group_create with it as a member.
 * pm_batchpir_dummy_preprocessing stays allowed (it only zeroes hints).  Before
 * its first completed stream (or dummy preprocessing) pm_batchpir_client_begin
 * is refused: "not preprocessed".  Where pm_batchpir_client_finish's
 * re-preprocessing trigger would preprocess, the handle cannot: finish returns
 * its results, pm_batchpir_prep_due becomes 1 and the next begin is refused,
 * "preprocessing due: stream it first"; after the stream the state and counters
 * equal those of a pm_batchpir_create_client twin after the Query that
 * re-preprocessed.  PM_EINVAL before any HIP call: ctx or out NULL, DBSize 0,
 * DBEntryByteNum < 8, BatchSize < 2.  Device memory: the hint state, tabT, cur
 * and, from the first stream on, two window slots of at most max(8 MiB, the
 * largest chunk). */
int pm_batchpir_create_remote(pm_ctx*, uint64_t DBSize, uint64_t DBEntryByteNum, uint64_t BatchSize,
                              uint64_t FailureProbLog2, uint64_t seed, pm_batchpir** out);
/* Streamed preprocessing: Piano's offline protocol, in which the DB passes the
 * client once, chunk by chunk, and is never stored.  The three calls work on a
 * remote handle and on any unsharded batch handle that has a DB (which it then
 * ignores: the reference's UpdatePreprocessing surface); a shard handle
 * (nshards > 1) is refused.
 * pm_batchpir_prep_stream_begin is Client.Initialization (pir.go:203-255) of
 * every partition: the next epoch's key, tags, program points, histogram and
 * PRF tables, zero parities and replacement values, default replacement
 * indices.  It opens a stream and closes an open split query, as
 * pm_batchpir_preprocessing does.  While the stream is open every client call
 * on the handle (pm_batchpir_client_begin / _finish, pm_batchpir_query*,
 * pm_batchpir_dummy_preprocessing, group calls, the graph calls over
 * pm_graph_pir) fails with PM_EINVAL, "a streamed preprocessing is open".  begin
 * on an open stream abandons it and starts over with the NEXT epoch: this is
 * how a dropped connection recovers, and it costs an epoch (the handle then
 * equals a twin that preprocessed once more).  pm_batchpir_preprocessing on a
 * handle with a DB also abandons an open stream.
 * pm_batchpir_prep_stream_rows is PianoPIRClient.UpdatePreprocessing
 * (pir.go:303-352) of chunks [chunk0, chunk0 + nchunks) of one partition in one
 * call.  rows: that range's existing rows, partition rows [chunk0 * ChunkSize,
 * min((chunk0 + nchunks) * ChunkSize, DBSize(P))), DBEntrySize words each
 * (pm_batchpir_subconfig gives ChunkSize, SetSize and DBSize(P)); nrows must be
 * their number, 0 (rows may be NULL) for chunks wholly past the partition's end,
 * which exist because SetSize is rounded up to a multiple of 4 and still get
 * their replacement indices.  The library zero-pads (pir.go:285-295).  Windows
 * may come in any order, from any partition and in any sizes; every chunk of
 * every partition exactly once.  rows is copied before the call returns and
 * never retained; the call does not wait for the device, so the upload of one
 * window overlaps the fold of the one before (sub-windows of whole chunks of at
 * most max(8 MiB, one chunk) through two pinned slots).  PM_EINVAL before any
 * HIP call and with nothing changed: a NULL handle, no open stream, "partition
 * out of range", nchunks 0, chunk0 + nchunks > SetSize, a wrong nrows, NULL rows
 * with nrows > 0, "chunk already delivered" for any overlap with an earlier
 * window.
 * pm_batchpir_prep_stream_end: PM_EINVAL "chunks missing: partition p, chunk c"
 * (the first one) while a chunk is undelivered, the stream staying open;
 * otherwise it waits for the device, closes the stream and resets the batch
 * counters and counts PrepCount as pm_batchpir_preprocessing does.  The handle
 * then equals, bit for bit in pm_batchpir_export and the counters of
 * pm_batchpir_stats_get, a pm_batchpir_create_client twin of the same seed after
 * the same number of pm_batchpir_preprocessing calls.  A HIP failure in rows or
 * end leaves the stream unusable: begin again.
 * Timing names: "prep_stream_fold", "prep_stream_repl" (level 1, one per
 * sub-window), "host_prep_stream" (wall time begin to end, one entry per
 * completed stream), "host_prep_stream_windows" (a count of sub-windows).
 * pm_set_option("stream_upload_only", 1) (probes): the sub-windows go through
 * the same staging but the two kernels are not launched; the hints are then
 * meaningless. */
int pm_batchpir_prep_stream_begin(pm_batchpir* h);
int pm_batchpir_prep_stream_rows(pm_batchpir* h, uint32_t partition, uint32_t chunk0, uint32_t nchunks,
                                 const uint64_t* rows, uint64_t nrows);
int pm_batchpir_prep_stream_end(pm_batchpir* h);
int pm_batchpir_prep_due(pm_batchpir* h);          /* 1 / 0; 0 for NULL */
/* the server's side of the stream: rows of chunks [chunk0, chunk0+nchunks) of one partition */
/* pm_batchpir_server_answer's sibling: copies, device to host, the rows
 * pm_batchpir_prep_stream_rows takes for that range into rows and sets *nrows
 * to their number (defined above; 0 for chunks past the end).  cap_rows < that
 * number gives PM_EINVAL with *nrows set.  Reads the DB only: it works on a
 * handle never preprocessed, on a client handle and on pm_graph_pir(g), and
 * touches no client state.  PM_EINVAL: a NULL handle or nrows, "no DB on this
 * handle", a partition out of range or not on this shard, nchunks 0, chunk0 +
 * nchunks > SetSize. */
int pm_batchpir_server_rows(pm_batchpir* h, uint32_t partition, uint32_t chunk0, uint32_t nchunks,
                            uint64_t* rows, uint64_t cap_rows, uint64_t* nrows);
/* The speculation record of this handle's last step (test hook), where the
 * fused step kernel (k_step, "host_path_step") ran it on a context created with
 * PM_STEP_SPEC=1: *nsub words in sub-query order (partition-major, qn slots per
 * partition) into out[0 .. cap).  k_step's answers start on a guess of their
 * resolution; each word says what became of one:
 *   bits 0-2  the guessed answer mode: 1 final, 4 dummy, 7 no guess
 *   bit  3    helped: the guessed set was gathered with the gather helpers
 *   bit  4    help_ok: every helper's guess was the answer's (1 where not helped)
 *   bit  5    kept: the resolution equals the guess in every field the answer reads
 *   bit  6    redo: the set was gathered again for the resolution (!kept || !help_ok)
 *   bits 8-10 the resolution's answer mode: 0 zero (failed / skipped), 1 final,
 *             2 chained (its hint was refreshed earlier in the step), 3 cached, 4 dummy
 *   bit  31   written by the kernel (always 1)
 * out NULL with cap 0: *nsub alone.  PM_EINVAL for a NULL argument otherwise, a
 * context without the record, a last step that did not run k_step (or none
 * yet), or cap < *nsub (*nsub is set). */
int  pm_batchpir_step_spec(pm_batchpir* h, uint32_t* out, uint64_t cap, uint64_t* nsub);

/* State export of one partition's client (test hook; sizes from the config):
 * round_keys[44], primary_tag[PH], primary_parity[PH*E], primary_pp[PH],
 * backup_tag[SS*Qpc], backup_parity[SS*Qpc*E], repl_idx[SS*Qpc],
 * repl_val[SS*Qpc*E], hist[SS].  Any pointer may be NULL. */
int pm_pir_export(pm_pir* h, uint32_t* round_keys, uint64_t* primary_tag, uint64_t* primary_parity,
                  uint64_t* primary_pp, uint64_t* backup_tag, uint64_t* backup_parity,
                  uint64_t* repl_idx, uint64_t* repl_val, uint64_t* hist);
int pm_batchpir_export(pm_batchpir* h, uint64_t partition, uint32_t* round_keys,
                       uint64_t* primary_tag, uint64_t* primary_parity, uint64_t* primary_pp,
                       uint64_t* backup_tag, uint64_t* backup_parity, uint64_t* repl_idx,
                       uint64_t* repl_val, uint64_t* hist);

/* ---- graphann (graphann/search.go) over PIRGraphInfo (private-search.go) */
/* PIRGraphInfo{N,Dim,M,graph,vectors,skipPrep,NonPrivateMode} (private-search.go:336-353)
 * wrapped in a GraphANNFrontend (search.go:69-72).  vectors: n x dim f32,
 * graph: n x m uint32.  nonprivate=1 gives BasicGraphInfo-style direct access
 * (private-search.go:445-455).  search_seed drives the host id stream that the
 * reference draws from global math/rand. */
int  pm_graph_create(pm_ctx* ctx, uint64_t n, uint64_t dim, uint64_t m, const float* vectors,
                     const uint32_t* graph, int nonprivate, int skip_prep, uint64_t pir_seed,
                     uint64_t search_seed, pm_graph** out);
void pm_graph_destroy(pm_graph* g);
int  pm_graph_preprocess(pm_graph* g);   /* GraphANNFrontend.Preprocess  search.go:74-81 */
/* GraphANNFrontend.SearchKNN (search.go:114-234); ids/steps: k entries, -1 padded */
int  pm_search_knn(pm_graph* g, const float* query, int k, int max_step, int parallel,
                   int benchmarking, int64_t* ids, int64_t* steps);
/* GraphANNFrontend.SearchKNNBatch (graphann/search.go:236-245): SearchKNN of
 * queries[i] for i = 0..nq-1 in order; ids/steps: nq x k, -1 padded.  The
 * result (ids, steps, pm_graph_counts, the id stream afterwards) is that of
 * the loop of pm_search_knn, for every graph and argument it accepts.  A
 * non-private in-memory graph is searched on the device, one workgroup per
 * query and all queries of a call in one launch ("knn_batch" at timing level
 * 1), when the search state fits the LDS (m <= 64, parallel * m <= 256, about
 * 36 B x parallel x (1 + max_step x m) rounded up to a power of two, within
 * 160 KB) and benchmarking is 0; a query whose search would draw from the id
 * stream (a pop on an empty heap) is re-run on the host in order
 * ("host_knn_batch_fallback").  *device_queries (nullable): the number of
 * queries answered by the kernel, 0 on the sequential path. */
int  pm_search_knn_batch(pm_graph* g, const float* queries, uint64_t nq, int k, int max_step,
                         int parallel, int benchmarking, int64_t* ids, int64_t* steps,
                         uint64_t* device_queries);
/* private-search.go:216-240 query loop incl. the maintenance trigger (:226-232) */
int  pm_search_loop(pm_graph* g, const float* queries, uint64_t q, int k, int step, int parallel,
                    int benchmarking, int64_t* answers, double* online_s, double* maintenance_s);
int  pm_graph_counts(pm_graph* g, uint64_t* total_queries, uint64_t* succ_queries);
/* A further client session over a preprocessed `base` (same graph, vectors and
 * server DB, shared on the device): own context/stream, PIR keys (pir_seed),
 * hint state, start set and id stream (search_seed).  Call pm_graph_preprocess
 * on it (client hint preprocessing + GetStartVertex) before searching. */
int  pm_graph_create_session(pm_ctx* ctx, pm_graph* base, uint64_t pir_seed, uint64_t search_seed,
                             pm_graph** out);
/* S sessions served concurrently on one GPU, one host thread each: session i
 * runs the private-search.go:216-240 loop (incl. its own maintenance trigger)
 * over queries[i*q*dim ...] into answers[i*q*k ...].  wall_s: wall time from the
 * common start to the last session's end; online_s / maintenance_s: S entries. */
int  pm_search_loop_sessions(pm_graph** sessions, uint32_t S, const float* queries, uint64_t q, int k,
                             int step, int parallel, int64_t* answers, double* wall_s, double* online_s,
                             double* maintenance_s);
/* The same sessions in lock-step with every batch-PIR round of all of them
 * fused into ONE shared step (k_match -> k_resolve ->
 * k_answer over S x 16 partitions, launched on sessions[0]'s stream): each
 * session keeps its own keys, hint state, cache, counters, search and
 * maintenance (private-search.go:216-240), and gets exactly the answers it
 * would get alone.  Sessions: clients of one server DB on one device (base +
 * pm_graph_create_session), distinct contexts.  ngroups (0: 1) lock-step
 * groups of consecutive sessions run concurrently, each with its own shared
 * steps on its first session's stream, so one group's step overlaps the
 * others' host work; nthreads host workers in all (0: min(S, 16)) run the
 * sessions' searches between the steps.  Outputs as pm_search_loop_sessions;
 * online_s[i] = wall_s - maintenance_s[i]. */
int  pm_search_loop_batched(pm_graph** sessions, uint32_t S, const float* queries, uint64_t q, int k, int step,
                            int parallel, uint32_t ngroups, uint32_t nthreads, int64_t* answers, double* wall_s,
                            double* online_s, double* maintenance_s);
pm_batchpir* pm_graph_pir(pm_graph* g);

/* ---- the GetGraphInfo plugin surface (graphann/search.go:20-25) ---------
 * PIRGraphInfo's methods as batch calls, for a caller that keeps its own beam
 * search (graphann.SearchKNN) and plugs the GPU in behind GetGraphInfo:
 *   pm_graph_preprocess       Preprocess()       private-search.go:355-412
 *   pm_graph_get_metadata     GetMetadata()      private-search.go (n, dim, m)
 *   pm_graph_get_vertex_info  GetVertexInfo(ids) private-search.go:441-506
 *   pm_graph_get_start_vertex GetStartVertex()   private-search.go:508-531
 *   pm_graph_group_*          GetVertexInfo / Preprocess of many sessions at once
 * pm_graph_get_vertex_info fetches every id through the batch PIR
 * (SimpleBatchPianoPIR.Query, one call per batch) and decodes the entries
 * (Entry2VectorAndNeighbors, :418-439) into vecs (n x dim f32) and nbrs
 * (n x m u32); a failed or dropped id decodes as zeros (ok[i] = 0), as in the
 * reference.  With a query (dim f32), dist[i] = L2Dist(vector i, query)
 * (build_graph.go:119-127, l2_distance_amd64.s order, 0 for a failed id) is
 * computed on the GPU next to the decode.  Any output may be NULL (dist needs
 * query).  Counts totalQueryNum / succQueryNum as the reference does
 * (pm_graph_counts).  pm_graph_get_start_vertex: the ⌊√n⌋ start vertices
 * chosen by pm_graph_preprocess (non-private), *count = their number, the
 * first min(cap, count) written. */
int pm_graph_get_metadata(pm_graph* g, uint64_t* n, uint64_t* dim, uint64_t* m);
int pm_graph_get_vertex_info(pm_graph* g, const uint64_t* ids, uint64_t n, float* vecs, uint32_t* nbrs, uint8_t* ok,
                             const float* query, float* dist);
int pm_graph_get_start_vertex(pm_graph* g, uint64_t cap, uint64_t* ids, float* vecs, uint32_t* nbrs,
                              uint64_t* count);
/* Many sessions' GetVertexInfo calls answered together: what
 * pm_batchpir_group_query is to SimpleBatchPianoPIR.Query, for a server whose
 * clients keep their own beam search.  Sessions: private, preprocessed,
 * unsharded clients of one server DB on one device with distinct contexts (a
 * base and its pm_graph_create_session handles, as pm_search_loop_batched
 * takes); PM_EINVAL with a message, before any HIP call, for a NULL, repeated,
 * non-private, sharded, lost or not preprocessed session and for sessions of
 * different devices or servers.  The group keeps the handles, which must
 * outlive it; its shared steps run on sessions[0]'s stream.  A session may be
 * used alone between group calls (never concurrently with one), and may be
 * re-preprocessed with pm_graph_preprocess: the next group call picks up its
 * new client.
 * pm_graph_group_get_vertex_info is, for every session s, exactly
 * pm_graph_get_vertex_info(sessions[s], ids + offs[s], offs[s+1] - offs[s],
 * ..., queries + s*dim, ...): the same vecs, nbrs, ok and dist at offs[s] (rows
 * of dim / m / 1 / 1 elements per id), the same pm_graph_counts, batch-PIR
 * statistics and hint state afterwards, bit for bit.  As there, a session's
 * ids are ONE SimpleBatchPianoPIR.Query; the sub-queries of all sessions go
 * into ONE shared step, with every row scored against its own session's query
 * (the S queries go to the device in one copy per call).  A session with
 * offs[s] == offs[s+1] sits the call out untouched.  A session whose bucketing
 * leaves the one-step path (a partition at its query budget, fewer ids than
 * partitions, more than 256 sub-queries per partition) is served alone in that
 * call, as pm_graph_get_vertex_info serves it, and the others still share the
 * step.  Any output may be NULL; dist needs queries (S x dim, or NULL).  offs
 * (S + 1 entries) must not descend; an id >= n of any session fails the whole
 * call (PM_EINVAL) before any session's state moves.
 * pm_graph_group_preprocess is pm_graph_preprocess of every session, the hint
 * folds of the sessions that are clients of a base as ONE launch set (as
 * pm_batchpir_group_preprocessing); every session's state equals that of its
 * own pm_graph_preprocess. */
typedef struct pm_graph_group pm_graph_group;
int  pm_graph_group_create(pm_graph** sessions, uint32_t S, pm_graph_group** out);
void pm_graph_group_destroy(pm_graph_group* gg);
int  pm_graph_group_get_vertex_info(pm_graph_group* gg, const uint64_t* ids, const uint64_t* offs /* S+1 */,
                                    float* vecs, uint32_t* nbrs, uint8_t* ok,
                                    const float* queries /* S x dim or NULL */, float* dist);
int  pm_graph_group_preprocess(pm_graph_group* gg);

/* ---- private search over a SHARDED graph DB (multi-GPU) --
 * The reference's PIRGraphInfo (private-search.go:336-531) fetches every
 * vertex record through SimpleBatchPianoPIR.Query (batch-pir.go:170-248),
 * whose 16 partitions are independent sub-PIRs (batch-pir.go:62-85): the
 * sharding axis.  Rank `shard` of `nshards` holds the partitions
 * p % nshards == shard (DB rows, keys, hint state) and runs the SAME sessions
 * (same seeds, same queries) as every other rank; each shared step's answers
 * are combined across the ranks so every rank continues identical searches.
 *
 * pm_graph_create_shard: host vectors (n x dim f32) and graph (n x m u32) as
 * pm_graph_create; only this shard's partitions are uploaded.
 * pm_graph_create_synth: the synthetic graph of the reference's
 * `-input synthetic` mode (private-search.go:42-69,114-117,168-170: uniform
 * [0,1) f32 vectors, uniform neighbour ids without self loops) as a pure
 * function of data_seed (pm_internal.h graph_synth_elem), generated on the
 * device: graph DBs of 10^8-10^9 entries that cannot be built or shipped.
 * pm_graph_synth_rows: the host restatement of those rows (vec / nb NULLable).
 * Sessions: pm_graph_create_session on a preprocessed base, as unsharded. */
int pm_graph_create_shard(pm_ctx* ctx, uint64_t n, uint64_t dim, uint64_t m, const float* vectors,
                          const uint32_t* graph, uint32_t shard, uint32_t nshards, uint64_t pir_seed,
                          uint64_t search_seed, pm_graph** out);
int pm_graph_create_synth(pm_ctx* ctx, uint64_t n, uint64_t dim, uint64_t m, uint64_t data_seed, uint32_t shard,
                          uint32_t nshards, uint64_t pir_seed, uint64_t search_seed, pm_graph** out);
int pm_graph_synth_rows(uint64_t n, uint64_t dim, uint64_t m, uint64_t data_seed, const uint64_t* ids, uint64_t k,
                        float* vec, uint32_t* nb);
/* The combine of one team's shared step: SUM-all-reduce (uint64, wrapping)
 * the nwords device words at dev_words in place across the ranks, ordered on
 * `stream` (a hipStream_t: the reduction waits for the stream's work and the
 * stream's later work waits for the reduction).  Every rank calls it for the
 * same (round, team) sequence.  0 = success. */
typedef int (*pm_combine_fn)(void* user, uint32_t team, uint64_t* dev_words, uint64_t nwords, void* stream);
/* Words of one team's records: sessions x parallel x m x W (W = the entry
 * words holding the neighbour list, + 1 for {dist, ok}), + 1 error word.  The
 * error word is 0 from a healthy rank and 1 from a rank whose team failed: such
 * a rank still takes the team's next combine turn (zero records, error word 1),
 * and every rank stops the team at that turn with PM_EHIP, so no rank is left
 * waiting inside a collective. */
uint64_t pm_sharded_record_words(pm_graph* g, uint32_t sessions, int parallel);

/* The library-native combine (replaces the per-step hop into the caller's
 * runtime, e.g. torch.distributed): RCCL communicators over xGMI, one per
 * lock-step team, created inside libpacmann.so from `nteams` ncclUniqueIds
 * that rank 0 makes (pm_rccl_unique_id) and the caller broadcasts over any
 * channel; pm_rccl_combine is a pm_combine_fn (user = the pm_rccl handle):
 * ncclAllReduce(ncclUint64, ncclSum) in place on the team's stream.  RCCL is
 * loaded on first use (dlopen of librccl.so.1, the copy already mapped into
 * the process if any).  The batch-pir.go:62-85 partitions are the shards; the
 * all-reduce is the north_star's final XOR-reduce (one rank answers each id,
 * so the integer sum is the XOR). */
#define PM_RCCL_ID_BYTES 128
typedef struct pm_rccl pm_rccl;
int  pm_rccl_unique_id(uint8_t id[PM_RCCL_ID_BYTES]);
int  pm_rccl_create(int device, int nranks, int rank, const uint8_t* ids /* nteams x PM_RCCL_ID_BYTES */,
                    uint32_t nteams, pm_rccl** out);
void pm_rccl_destroy(pm_rccl* r);
int  pm_rccl_combine(void* user, uint32_t team, uint64_t* dev_words, uint64_t nwords, void* stream);
/* Creation is bounded, by one path: the teams' communicators are created
 * nonblocking (ncclCommInitRankConfig, blocking = 0) inside ONE
 * ncclGroupStart / ncclGroupEnd group, and each one's state is polled (with a
 * sleep between polls) for at most pm_set_option("rccl_timeout_s") seconds
 * (else PM_RCCL_TIMEOUT_S, default 120).  A rank whose peer never joins gets
 * PM_ETIMEDOUT, not a hang.  Its communicators are aborted (ncclCommAbort), so
 * no thread of the library stays inside RCCL.  An RCCL without the nonblocking
 * API gives PM_EHIP.
 * pm_rccl_probe runs one 1-word all-reduce per team within the same bound and
 * checks that it sums to nranks; on failure the communicators are aborted.
 * Callers agree on the ranks' outcomes over another channel (a MIN of their
 * success flags) and fall back to another combine unless every rank
 * succeeded (pacmann_amd.shard.RcclCombiner.prepare). */
int  pm_rccl_probe(pm_rccl* r);
/* pm_search_loop_batched over a sharded graph DB: S sessions (clients of one
 * shard's server DB) in ngroups lock-step teams; every round of a team is one
 * shared step over this shard's partitions followed by ONE combine of the
 * team's per-id records {neighbour list, L2 distance to the session's query,
 * success flag} (zero where this shard holds no answer: exactly one shard
 * answers an id, so the sum is the unsharded answer bit for bit).  Teams issue
 * their combines in one global (round, team) order on every rank.
 * team_bufs: NULL (library buffers) or one device buffer per team of
 * pm_sharded_record_words(sessions of that team) words (the tensors a
 * torch.distributed combine reduces in place); team g = sessions
 * [S*g/ngroups, S*(g+1)/ngroups).  combine NULL: no exchange, valid when this
 * shard holds every partition, or with model_peers = 1 (synthetic graphs
 * only): the other shards' partitions are answered from the graph's spec on
 * the device (a wider shard layout measured one shard per GPU; modelled).
 * Outputs as pm_search_loop_batched; the answers are identical on every rank
 * and equal to the unsharded search's. */
int pm_search_loop_sharded(pm_graph** sessions, uint32_t S, const float* queries, uint64_t q, int k, int step,
                           int parallel, uint32_t ngroups, uint32_t nthreads, pm_combine_fn combine, void* user,
                           uint64_t* const* team_bufs, int model_peers, int64_t* answers, double* wall_s,
                           double* online_s, double* maintenance_s);

/* ---- graph construction + ground truth (graphann/build_graph.go) ------- */
/* Exact k nearest base rows of each query by (L2Dist, id), k <= 64: the
 * ground truth ComputeRecall (build_graph.go:821-863) scores against.  ids:
 * nq x k (-1 padded), dists: nq x k or NULL.  Exact for integer-valued rows
 * (e.g. SIFT's uint8 values); for general float rows the GPU keeps the 64 best
 * by bf16-rounded distance before the exact re-rank, so the result can differ
 * from brute force: pm_knn_exact is exact for those too. */
int pm_knn(pm_ctx* ctx, const float* base, uint64_t n, uint64_t dim, const float* queries, uint64_t nq,
           uint32_t k, int64_t* ids, float* dists);
/* pm_knn, exact for every finite float input: the result is the brute-force
 * (L2Dist in l2_distance_amd64.s order, id) ranking.  The prefilter splits
 * every row into two bf16 halves and bounds its own error (eps <= 2^-12 (|q|^2 +
 * max |x|^2)); a query row whose k-th exact distance lies more
 * than eps below the prefilter distance of its 64th candidate is certified,
 * every other row is answered again by a brute-force kernel (slow: n dim
 * operations per row).  *fallback_rows (nullable): rows answered by the
 * brute-force kernel instead of the certified prefilter.  Non-finite inputs
 * get some answer through the fallback.  Arguments as pm_knn; dim <= 192
 * (pm_knn_wide takes rows up to 1,024). */
int pm_knn_exact(pm_ctx* ctx, const float* base, uint64_t n, uint64_t dim, const float* queries, uint64_t nq,
                 uint32_t k, int64_t* ids, float* dists, uint64_t* fallback_rows);
/* BuildGraph / CreateGraphBasedOnNGT (build_graph.go:97-105,314-523) with the
 * NGT candidate search (absent here) replaced by exact kNN: candidates =
 * int(1.5 m) nearest by (L2Dist, id) minus u; robustPrune (alpha); reverse
 * edges; edge sampling with probability min(1.5 m / inbounds, 1); second
 * robustPrune; random fill to exactly m.  Sampling and fill draw from
 * hash4(seed, ...).  graph: n x m.  times (NULL or 4
 * doubles): kNN, first prune, host edge work, second prune, in seconds.
 * dim <= 192, m <= 42. */
int pm_build_graph(pm_ctx* ctx, const float* vectors, uint64_t n, uint64_t dim, uint64_t m, float alpha,
                   uint64_t seed, uint32_t* graph, double* times);
/* pm_build_graph with pm_knn_exact's candidates: equals the oracle's graph for
 * float rows too.  *fallback_rows (nullable): vertices whose candidates came
 * from the brute-force kernel.  Other arguments as pm_build_graph. */
int pm_build_graph_exact(pm_ctx* ctx, const float* vectors, uint64_t n, uint64_t dim, uint64_t m, float alpha,
                         uint64_t seed, uint32_t* graph, double* times, uint64_t* fallback_rows);
/* Test probes of the two calls above (tests/test_gpu_knn_stages.py,
 * tests/test_gpu_prune.py): the same uploads and kernel launches, with the
 * values the product drops copied out.
 * pm_knn_stages runs pm_knn (exact = 0) or pm_knn_exact (exact != 0) for k and
 * returns, per query row, the prefilter's 64 candidate ids in key order (cand
 * nq x 64, 0xffffffff for an empty slot) and their prefilter distances (pref
 * nq x 64, all-ones bits for an empty slot); both are required.  For exact it
 * also fills whichever of these is not NULL: tau [nq] (the 64th prefilter
 * distance; NaN bits with fewer than 64 base rows), eps [nq] (the bound the
 * row was judged with; NaN bits for n <= 64, where no row is judged), qnorm
 * [nq] and bnorm [n] (the norms), maxnorm (the bits of the largest base norm),
 * bhi / blo (the bf16 halves of the base rows, n x dp, zero padded),
 * uncertified [nq] (the rows that went to the brute-force kernel, ascending;
 * their number in n_uncertified = pm_knn_exact's fallback_rows).  dp: the
 * padded row width (128 or 192).  PM_EINVAL as pm_knn_exact, and for nq = 0. */
typedef struct pm_knn_stages_out {
  uint32_t* cand;
  float* pref;
  float *tau, *eps, *qnorm, *bnorm;
  uint32_t* maxnorm;
  uint16_t *bhi, *blo;
  uint64_t* uncertified;
  uint64_t n_uncertified;
  uint32_t dp;
} pm_knn_stages_out;
int pm_knn_stages(pm_ctx* ctx, const float* base, uint64_t n, uint64_t dim, const float* queries, uint64_t nq,
                  uint32_t k, int exact, pm_knn_stages_out* out);
/* pm_robust_prune runs robustPrune (build_graph.go:169-236) on the GPU as the
 * build's second pass does: list b is ids[offs[b] .. offs[b] + lens[b]), the
 * candidates of vertex verts[b] (distinct vertices, ids < n; nids entries in
 * ids).  presorted = 0: every list by the kernel's own sort, which holds 4,096
 * candidates; a longer list sets *err to 1 and gets length 0.  presorted != 0:
 * every list by the form the build uses for longer lists (distances on the
 * GPU, sorted on the host, the same greedy pass).  out: nverts x m (row b holds
 * out_len[b] ids).  m <= 64, dim <= 256. */
int pm_robust_prune(pm_ctx* ctx, const float* vectors, uint64_t n, uint64_t dim, const uint32_t* verts,
                    uint64_t nverts, const uint64_t* offs, const uint32_t* lens, const uint32_t* ids, uint64_t nids,
                    uint32_t m, float alpha, int presorted, uint32_t* out, uint32_t* out_len, uint32_t* err);

/* ---- rows up to 1,024 dimensions --------------------- */
/* The four calls below are pm_knn_exact, pm_build_graph_exact, pm_knn_stages
 * (exact form) and pm_robust_prune for dim in [1, 1024]; every other argument
 * rule is the narrow call's (k in [1, 64]; m in [1, 42] for the build and
 * [1, 64] for the prune probe).  dim = 0 or dim > 1024 gives PM_EINVAL, "dim
 * must be in [1, 1024]", before any HIP call.  For dim <= 192 they run the
 * narrow calls' kernels unchanged, so a caller needs only these names.  For
 * dim in [193, 1024] the rows are padded to the next multiple of 64 (dp) and
 * the prefilter walks them in chunks of 64 (k_knn_bf16x3_w, timing name
 * "knn_prefilter_w"); the fallback and robustPrune keep one row in LDS
 * (k_knn_brute<64, 1024>, k_prune<false>).  Only the exact (certified) form exists for wide
 * rows: pm_knn's promise for integer rows needs dim * 255^2 < 2^24, i.e. dim
 * <= 258.  The certificate's eps is c_dp (|q|^2 + max |x|^2) + 2^-50 with c_dp =
 * 2 (3 dp + 8) 2^-23 + 2^-16 (1 + 2^-6) + 2^-17: 2.08e-4 at dp 256, 3.91e-4 at
 * 512, 7.57e-4 at 1,024, above the 2^-12 quoted for the narrow path, so wide
 * rows reach the brute-force kernel more often on tightly clustered data.
 * The result is the brute-force (L2Dist in l2_distance_amd64.s order, id)
 * ranking for every finite float input either way. */
int pm_knn_wide(pm_ctx* ctx, const float* base, uint64_t n, uint64_t dim, const float* queries, uint64_t nq,
                uint32_t k, int64_t* ids, float* dists, uint64_t* fallback_rows);
/* pm_build_graph_exact for dim in [1, 1024], m <= 42: equals the oracle's graph. */
int pm_build_graph_wide(pm_ctx* ctx, const float* vectors, uint64_t n, uint64_t dim, uint64_t m, float alpha,
                        uint64_t seed, uint32_t* graph, double* times, uint64_t* fallback_rows);
/* Test probes: pm_knn_stages' exact form (out->dp reports the padded width:
 * 128, 192 or the next multiple of 64) and pm_robust_prune. */
int pm_knn_stages_wide(pm_ctx* ctx, const float* base, uint64_t n, uint64_t dim, const float* queries, uint64_t nq,
                       uint32_t k, pm_knn_stages_out* out);
int pm_robust_prune_wide(pm_ctx* ctx, const float* vectors, uint64_t n, uint64_t dim, const uint32_t* verts,
                         uint64_t nverts, const uint64_t* offs, const uint32_t* lens, const uint32_t* ids,
                         uint64_t nids, uint32_t m, float alpha, int presorted, uint32_t* out, uint32_t* out_len,
                         uint32_t* err);

/* ---- 128 prefilter keys per query row ----------------- */
/* pm_knn_wide, pm_build_graph_wide and pm_knn_stages_wide with 128 instead of
 * 64 prefilter keys per query row, for every k and m: k in [1, 128] ("k must be
 * in [1, 128]") and, in the build, m in [1, 64] ("m must be in [1, 64]": int(1.5
 * m) + self = 97 keys); dim in [1, 1024] and every other rule as the _wide
 * calls', all checked before any HIP call.  The prefilter distances are the
 * 64-key kernels' bit for bit and eps is unchanged; tau is the 128th prefilter
 * distance instead of the 64th, so for k <= 64 the uncertified rows are a subset
 * of pm_knn_wide's: a caller who wants fewer brute-force rows gets them by
 * name.  Rows with n <= 128 are never judged.  Timing names: "knn_prefilter_k128"
 * (dp 128 / 192), "knn_prefilter_k128_w" (dp 256 .. 1,024, K chunks of 32),
 * "knn_rerank", "knn_brute".  The result is the brute-force (L2Dist in
 * l2_distance_amd64.s order, id) ranking, -1 / +inf padded, for every finite
 * float input. */
int pm_knn_k128(pm_ctx* ctx, const float* base, uint64_t n, uint64_t dim, const float* queries, uint64_t nq,
                uint32_t k, int64_t* ids, float* dists, uint64_t* fallback_rows);
/* pm_build_graph_wide for m in [1, 64]: equals the oracle's graph. */
int pm_build_graph_k128(pm_ctx* ctx, const float* vectors, uint64_t n, uint64_t dim, uint64_t m, float alpha,
                        uint64_t seed, uint32_t* graph, double* times, uint64_t* fallback_rows);
/* Test probe: pm_knn_stages_wide with out->cand and out->pref [nq][128]; eps
 * holds NaN bits where no row was judged (n <= 128). */
int pm_knn_stages_k128(pm_ctx* ctx, const float* base, uint64_t n, uint64_t dim, const float* queries, uint64_t nq,
                       uint32_t k, pm_knn_stages_out* out);
uint32_t pm_knn_k128_top(void);   /* 128 */

/* ---- uint8 rows on the int8 matrix cores -------------- */
/* pm_knn and pm_build_graph for rows of bytes (SIFT / BIGANN .bvecs), which go
 * to the device as bytes.  For values 0..255 and dim <= 256 every squared
 * distance is an integer <= 256 * 255^2 < 2^24, so every term and partial sum of
 * L2Dist is exact in f32 in any order: the integer distance converted to float
 * is the reference's L2Dist bit for bit, and the (integer distance, id) ranking
 * is the (L2Dist, id) ranking.  That is where the limit comes from: dim in
 * [1, 256] ("dim must be in [1, 256]").  There is no re-rank, no certificate
 * and no fallback, hence no fallback_rows.  k in [1, 128] ("k must be in [1,
 * 128]"), n in [1, 2^32-1) ("n must be in [1, 2^32-1)"), ids -1 and dists +inf
 * padded for k > n, dists may be NULL; all rules are checked before any HIP
 * call.  Device memory of the kNN call: n dp + 4 n bytes for the base (dp: dim
 * rounded up to a multiple of 64), the same for the queries, and a staging
 * buffer of at most 32 MiB.  Timing names: "u8_bias", "knn_prefilter_u8". */
int pm_knn_u8(pm_ctx* ctx, const uint8_t* base, uint64_t n, uint64_t dim, const uint8_t* queries, uint64_t nq,
              uint32_t k, int64_t* ids, float* dists);
/* pm_build_graph_k128 for byte rows, m in [1, 64] ("m must be in [1, 64] ..."),
 * n > m: the candidates come from the integer kNN; the robustPrune stages, the
 * host edge work and the fill are pm_build_graph's, over an f32 copy of the rows
 * made on the device ("u8_to_f32"), so the build (not the kNN call) also holds
 * n dim 4 bytes there.  times as pm_build_graph's four.  Equals the oracle's
 * graph of the rows as floats. */
int pm_build_graph_u8(pm_ctx* ctx, const uint8_t* vectors, uint64_t n, uint64_t dim, uint64_t m, float alpha,
                      uint64_t seed, uint32_t* graph, double* times);
uint32_t pm_knn_u8_max_dim(void);   /* 256 */

/* ---- k-means and the cluster-search baseline ---------- */
/* Deterministic Lloyd iterations (the clustering() of the reference's
 * cluster-search.py:88-107, which calls faiss.Kmeans(niter=20) and then
 * index.search(vectors, 1)).  dim in [1, 1024] ("dim must be in [1, 1024]"),
 * n in [1, 2^32-1) ("n must be in [1, 2^32-1)"), nc in [1, n] ("nc must be in
 * [1, n]"), niter in [0, 10000] ("niter must be in [0, 10000]"); ctx, vectors,
 * centroids and labels not NULL; all checked before any HIP call.
 *
 * Start: init [nc][dim] as given, or, when it is NULL, centroid c = row pick[c],
 * pick the first nc entries of a Fisher-Yates shuffle of 0 .. n-1 whose i-th
 * swap partner is i + hash4(seed, 12, i, 0, 0) % (n - i) (O(nc) host memory).
 * This is not faiss's sampling: the reference seeds faiss from its own RNG and
 * is not reproducible between runs anyway; faiss's empty-cluster splitting and
 * its sub-sampling of the training points are not done either.
 *
 * Assignment: labels[i] = the c that minimises (L2Dist(row i, centroid c), c),
 * L2Dist in l2_distance_amd64.s order, ties to the lowest c, exact for every
 * finite input: pm_knn_k128's device path with the centroids as base, the rows
 * as queries and k = 1 (timing names as pm_knn_k128's).  The rows' bf16 halves
 * and norms are made once per call, the centroids' each iteration.
 *
 * Update: centroid c becomes the mean of its members, or keeps its value when it
 * has none.  Coordinate j of the mean: the members in ascending id order; partial
 * sum p of 16 adds members p, p + 16, ... in that order in f64 from +0.0; the
 * total is partial 0 plus partials 1 .. 15 in that order; total / size in f64,
 * rounded once to f32.  This order is part of the contract: the result is a
 * function of the input alone (no floating-point atomics, nothing that depends
 * on scheduling), and two calls return the same bits.
 *
 * Loop: assign; then niter times: update, assign.  labels is always the
 * assignment to the returned centroids.  moved [niter + 1] (or NULL): moved[t] =
 * the rows whose label changed in assignment t, moved[0] = n; when an assignment
 * moves nothing the loop stops (the centroids are a fixed point) and the
 * remaining entries are 0.  sizes [nc] (or NULL): the final member counts.
 * niter = 0 labels the rows by the given centroids.
 *
 * Device memory at the peak: n (4 dim + 4 dp + 12) bytes for the rows, their two
 * bf16 halves (dp: dim padded as pm_knn_k128 pads it), norms and two label
 * arrays; 20 n bytes plus rocPRIM's sort scratch (about 16 n) for the member
 * lists; nc (4 dim + 4 dp + 4) for the centroids; and about 540 bytes per row of
 * an assignment chunk of at most 262,144 rows (142 MB), whatever n is.  Timing
 * names of the stages that are not the kNN's: "kmeans_sort" (the member lists),
 * "kmeans_update", "kmeans_moved". */
int pm_kmeans(pm_ctx* ctx, const float* vectors, uint64_t n, uint64_t dim, uint64_t nc, uint32_t niter,
              uint64_t seed, const float* init /* nc x dim or NULL */, float* centroids /* nc x dim */,
              uint32_t* labels /* n */, uint64_t* sizes /* nc or NULL */, uint64_t* moved /* niter + 1 or NULL */);

/* The cluster-ordered index of cluster-search.py (cluster_search_index,
 * :110-198) on the device.  pm_cluster_create takes centroids [nc][dim] and
 * labels [n] from anywhere (pm_kmeans, or the reference's saved -centroids.npy /
 * -labels.npy); dim and n as pm_kmeans, nc in [1, 2^32-1), a label >= nc is
 * PM_EINVAL ("label out of range"), all before any HIP call.  It keeps on the
 * device the rows gathered into cluster order (sorted_vectors, :122-131; within a
 * cluster by ascending id; "cluster_sort", "cluster_gather"), order [n] (the
 * original id of every position), and the centroids with their bf16 halves;
 * offsets [nc + 1] and a copy of order stay on the host (pm_cluster_info; any
 * output may be NULL).  Device memory held: n (4 dim + 4) + nc (4 dim + 4 dp + 4)
 * bytes; twice the rows during the create.  The context must outlive the index.
 *
 * pm_cluster_search: k in [1, 128] ("k must be in [1, 128]"), nq >= 1 ("nq must
 * be > 0"), nprobe in [1, min(nc, 128)] ("nprobe must be in [1, min(nc, 128)]").
 * probed [nq][nprobe] (or NULL) = the nprobe nearest centroids of each query by
 * (L2Dist, c), exact (pm_knn_k128's device path).  ids [nq][k] = the k smallest
 * (L2Dist(row, query), original id) keys over the union of the probed clusters'
 * rows, dists [nq][k] (or NULL) their distances, -1 / +inf padded as the kNN
 * calls'; scanned [nq] (or NULL) = the rows scored (the sum of the probed
 * sizes).  Timing names: "cluster_scan" and "cluster_merge", once per 65,536
 * queries, beside the kNN's.
 *
 * Departures from the script: distances are the graph side's squared L2Dist (the
 * script's np.linalg.norm gives the same ranking, not the same bits); ties break
 * by id (the script's argsort is unstable); a cluster shorter than k pads with
 * -1 (the script repeats the cluster's first row); nprobe > 1 is an extension
 * (Tiptoe's search is nprobe = 1). */
typedef struct pm_cluster pm_cluster;
int pm_cluster_create(pm_ctx* ctx, const float* vectors, uint64_t n, uint64_t dim, const float* centroids,
                      uint64_t nc, const uint32_t* labels, pm_cluster** out);
void pm_cluster_destroy(pm_cluster* h);
int pm_cluster_info(pm_cluster* h, uint64_t* n, uint64_t* dim, uint64_t* nc, uint64_t* offsets /* nc + 1 or NULL */,
                    uint32_t* order /* n or NULL */);
int pm_cluster_search(pm_cluster* h, const float* queries, uint64_t nq, uint32_t k, uint32_t nprobe,
                      int64_t* ids /* nq x k */, float* dists /* nq x k or NULL */,
                      uint32_t* probed /* nq x nprobe or NULL */, uint64_t* scanned /* nq or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* PACMANN_H */
