// pm_engine.h — what more than one of pm_engine.cpp, pm_search.cpp,
// pm_group.cpp and pm_devloop.cpp needs: the engine, graph-session and
// step-group types with their inline helpers, and the declarations (namespace
// pmh) of what one of these files uses of another.  Internal to those four:
// pm_ctx.cpp, pm_rccl.cpp and pm_build.cpp include pm_host.h alone.
#pragma once
#include "pm_host.h"

#include <functional>

struct DbGen;
struct Engine;
struct pm_graph;
struct StepGroup;
struct StepBufs;
struct ShardComb;

// ---------------------------------------------------------------------------
// Functions used across these files.  Each is defined once, in the file named
// above its group; what one file alone uses is static there and is not listed.
// ---------------------------------------------------------------------------
namespace pmh {
// pm_engine.cpp
int engine_create(pm_ctx* ctx, Engine* g, uint64_t N, uint64_t Ebytes, uint64_t B,
                  const uint64_t* rawDB, uint64_t F, uint64_t seed, bool batch,
                  uint32_t shard = 0, uint32_t nshards = 1, const Engine* server = nullptr,
                  const DbGen* gen = nullptr, uint32_t coord_words = 0, bool remote = false);
int ensure_host_cache(Engine* g);
int engine_prep_host(Engine* g, uint64_t p0, uint64_t p1, std::vector<uint64_t>& todo,
                     hipStream_t st = nullptr);
int engine_prep_launch(pm_ctx* c, const Engine* g, const PmPart* dp, int np, const PmPart* host_parts,
                       uint32_t clients = 1, bool sync = true);
int wait_done(pm_ctx* sc, uint64_t seq);
int poll_done(pm_ctx* sc, uint64_t seq, bool* ready);
int wait_step(pm_ctx* c, const PmOutHdr* hdr, uint32_t nsub, uint32_t token, const char* rows,
              size_t row_bytes, size_t pf_off, size_t pf_len, uint64_t seq, pm_ctx* sc = nullptr);
void post_results(Engine* g, PmOutHdr* hdr, uint64_t* rows, uint32_t nsub, uint32_t base,
                  uint32_t token);
constexpr int kChainStop = 1 << 30;   // after_resolve's return value that ends the chain there, with success
int step_chain(pm_ctx* c, StepBufs& B, PmStep& S, const pmk::StepShape& shape, uint32_t nreal, double ans_bytes,
               const std::function<int()>& after_resolve = {});
int engine_step(Engine* g, const float* q_dev, uint32_t dim);
// PM_EINVAL while the engine has an open split query ("a split query is open") or an open streamed
// preprocessing ("a streamed preprocessing is open"): the first check of every client call
int client_guard(const Engine* g);
int db_guard(const Engine* g);   // PM_EINVAL "no DB on this handle" for a remote engine (pm_batchpir_create_remote)
void print_stamps(const Engine& e);
void record_stats(Engine* g, double t);
int batch_prep(Engine* g);
int batch_query(Engine* g, const uint64_t* idx, uint64_t n, uint64_t* out, const float* q_dev,
                uint32_t dim, float* dist_out, const uint64_t** rows_out = nullptr,
                uint8_t* ok = nullptr);
int bq_prepare(Engine* g, const uint64_t* idx, uint64_t n, bool* fast);
void bq_emit_fast(Engine* g, const uint64_t* idx, uint64_t n, uint64_t* out, float* dist_out,
                  const uint64_t** rows_out, uint8_t* ok);
int bq_tail(Engine* g, uint64_t n);
int batch_query_impl(Engine* g, const uint64_t* idx, uint64_t n, uint64_t* out, const float* q_dev,
                     uint32_t dim, float* dist_out, const uint64_t** rows_out, uint8_t* ok);
// pm_search.cpp
int check_session(const pm_graph* g);
int graph_start_set(pm_graph* g);
int gvi_pre(pm_graph* g, bool with_q, bool* fast);
int gvi_post(pm_graph* g, bool with_q, bool fast);
void knn_reset(pm_graph* g);
void knn_begin_finish(pm_graph* g, int parallel, int benchmarking, const float* sdh = nullptr);
void knn_batch(pm_graph* g, int parallel, int benchmarking);
void knn_update(pm_graph* g, int step);
void knn_end(pm_graph* g, int k, int64_t* ids_out, int64_t* steps_out);
// pm_group.cpp
int group_step_launch(StepGroup& G, PmStep& S, int kind, uint32_t max_per_part, uint32_t nreal, double ans_bytes);
int prep_clients(pm_ctx* c, DevBuf& pbuf, const std::vector<uint32_t>& lp, const std::vector<Engine*>& who,
                 const std::vector<double*>* mt, HostBuf* stage = nullptr, hipEvent_t* stage_ev = nullptr);
int team_init(StepGroup& G, pm_graph** gs, uint32_t S);
void team_release(pm_graph** gs, uint32_t S);
int run_batched_team(pm_graph** gs, uint32_t S, const float* queries, uint64_t q, int k, int step,
                     int parallel, uint32_t T, int64_t* answers, double* mt_out, ShardComb* comb = nullptr,
                     uint32_t team = 0);
hipStream_t team_stream(int dev, uint32_t t);
int run_batched_pool(pm_graph** gs, uint32_t S, const float* queries, uint64_t q, int k, int step, int parallel,
                     uint32_t NG, uint32_t T, int64_t* answers, double* mt_out);
// the two serving entry points' session checks and team threads
int check_loop_sessions(pm_graph** gs, uint32_t S, bool sharded);
using TeamFn = std::function<int(uint32_t g, uint32_t s0, uint32_t s1, uint32_t Tg)>;
int run_teams(pm_graph** gs, uint32_t S, uint32_t NG, uint32_t TT, const TeamFn& fn);
}  // namespace pmh

// Open-addressing uint64 -> uint32 map with O(1) clear (generation stamps).
// Replaces node-allocating std::unordered_map on the per-round host path
// (knownVertices, the batch response map, the per-partition localCache index).
// One 16-B slot {key, value, generation} per entry: a probe touches one cache
// line (the serving loop's session state is cold when its task runs, so the
// probes are cache misses; prefetch() issues a key's line ahead of a batch).
struct FlatMap {
  struct Slot { uint64_t key; uint32_t val, gen; };
  std::vector<Slot> slot;
  uint32_t cur = 1, count = 0, mask = 0;
  explicit FlatMap(uint32_t cap_pow2 = 256) { rehash(cap_pow2); }
  static uint64_t mix(uint64_t x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; return x; }
  void rehash(uint32_t cap) {
    std::vector<Slot> s0;
    s0.swap(slot);
    slot.assign(cap, Slot{0, 0, 0});
    mask = cap - 1; count = 0;
    const uint32_t old = cur; cur = 1;
    for (const Slot& x : s0) if (x.gen == old) put(x.key, x.val);
  }
  void clear() { if (++cur == 0) { for (Slot& x : slot) x.gen = 0; cur = 1; } count = 0; }
  void reserve(uint32_t n) { uint32_t c = (uint32_t)slot.size(); while (c < 2 * n) c *= 2; if (c != slot.size()) rehash(c); }
  void prefetch(uint64_t k) const { __builtin_prefetch(&slot[(uint32_t)mix(k) & mask]); }
  uint32_t* find(uint64_t k) {
    for (uint32_t i = (uint32_t)mix(k) & mask;; i = (i + 1) & mask) {
      Slot& x = slot[i];
      if (x.gen != cur) return nullptr;
      if (x.key == k) return &x.val;
    }
  }
  void put(uint64_t k, uint32_t v) {   // insert or overwrite
    if (2 * (count + 1) > slot.size()) rehash((uint32_t)slot.size() * 2);
    for (uint32_t i = (uint32_t)mix(k) & mask;; i = (i + 1) & mask) {
      Slot& x = slot[i];
      if (x.gen != cur) { x.gen = cur; x.key = k; x.val = v; ++count; return; }
      if (x.key == k) { x.val = v; return; }
    }
  }
  bool emplace(uint64_t k, uint32_t v) {   // insert if absent; true if inserted
    if (find(k)) return false;
    put(k, v);
    return true;
  }
  template <class F> void for_each(F&& f) const {
    for (const Slot& x : slot) if (x.gen == cur) f(x.key, x.val);
  }
};

// ---------------------------------------------------------------------------
// One step's scratch (k_match -> k_resolve -> [k_gather] -> k_answer), held by
// an Engine for its own steps and by a StepGroup for its shared ones.  The
// device buffers are sized by reserve() for nsub sub-queries over np
// partitions; part_x (split gather), qset, helpg, stamps (stamp builds) and the pinned
// descriptor / result buffers are reserved where a step needs them.
// ---------------------------------------------------------------------------
struct StepBufs {
  DevBuf subs_d, sb_d, bits, cand, meta, spec, res_d, ans, part_x, stamps;
  DevBuf qset;    // query sets expanded by k_match_resolve_s (PmStep::qset)
  DevBuf helpg;   // k_step's gather helpers' hand-off granules
  DevBuf specrec;           // k_step's speculation record (PmStep::specrec; contexts of PM_STEP_SPEC=1)
  uint32_t spec_nsub = 0;   // ... the sub-queries of the last step if k_step ran it with the record, else 0
  HostBuf desc_h, out_h;
  int reserve(uint32_t nsub, uint32_t np, uint32_t words, uint32_t cblk, uint64_t E) {
    CHK(subs_d.reserve(nsub * sizeof(PmSub)));
    CHK(sb_d.reserve((np + 1) * 4));
    CHK(bits.reserve((uint64_t)nsub * words * 8));
    CHK(cand.reserve((uint64_t)nsub * cblk * 6 * 4));
    CHK(meta.reserve((uint64_t)nsub * 2 * 4));
    CHK(spec.reserve((uint64_t)nsub * 64 * 4));
    CHK(res_d.reserve(nsub * sizeof(PmRes)));
    CHK(ans.reserve((uint64_t)nsub * E * 8));
    return 0;
  }
  void fill(PmStep& S, uint32_t words, uint32_t cblk) const {
    S.subs = subs_d.as<PmSub>();
    S.sb = sb_d.as<uint32_t>();
    S.bits = bits.as<uint64_t>();
    S.cand = cand.as<uint32_t>();
    S.meta = meta.as<uint32_t>();
    S.spec = spec.as<uint32_t>();
    S.res = res_d.as<PmRes>();
    S.ans = ans.as<uint64_t>();
    S.words = words;
    S.cblk = cblk;
  }
};
// A step's results for nsub sub-queries in one buffer (pinned, or device memory
// where they stay on the GPU): the headers, then the rows.
static inline size_t step_out_bytes(uint32_t nsub, uint64_t E) { return nsub * sizeof(PmOutHdr) + (size_t)nsub * E * 8; }
static inline void step_out(PmStep& S, void* out, uint32_t nsub) {
  S.hdr_h = (PmOutHdr*)out;
  S.rows_h = (uint64_t*)((char*)out + nsub * sizeof(PmOutHdr));
}
// The step's token: 0 never marks a published header.
static inline uint32_t next_token(uint32_t& token) {
  if (++token == 0) ++token;
  return token;
}
// The row words [pf_w0, pf_w1) the consumer reads next (bytes [pf_off, pf_off +
// pf_len) of each E-word row): checksummed in the header (PmOutHdr).
static inline void step_read_window(PmStep& S, size_t pf_off, size_t pf_len, uint64_t E) {
  const size_t off = std::min<size_t>(pf_off, E * 8);
  const size_t end = std::min<size_t>(E * 8, off + std::min<size_t>(pf_len, E * 8));
  S.pf_w0 = (uint32_t)(off / 8);
  S.pf_w1 = (uint32_t)((end + 7) / 8);
}
// PmStep::rows_partial for results the host reads: only the window's words are
// sent when the caller reads no others, unless a diagnostic re-reads whole rows.
static inline uint32_t host_rows_partial(const pm_ctx* c, bool partial) {
  return partial && !c->verify_rows && !c->debug_cache ? 1u : 0u;
}
// ---------------------------------------------------------------------------
// PianoPIR engine: P partitions (P = 1 for PianoPIR, BatchSize/2 for the batch)
// ---------------------------------------------------------------------------
struct PartHost {
  PmPart d{};
  bool owned = true;   // sharded engines hold the state of their own partitions only
  uint64_t epoch_ctr = 0, fqn = 0, dummy_ctr = 0;
  uint64_t maxq64 = 0;
  FlatMap cache;   // localCache (pir.go:120): idx -> arena slot
  std::unordered_map<uint64_t, std::vector<uint64_t>> shadow;   // PM_DEBUG_CACHE: slot -> row the host got
};

struct Engine {
  pm_ctx* ctx = nullptr;
  // a serial number per process: pm_graph_preprocess re-creates a session's client, possibly at the same
  // address, and a pm_graph_group that copied the old one's parts must notice
  static uint64_t next_uid() { static std::atomic<uint64_t> n{0}; return ++n; }
  const uint64_t uid = next_uid();
  bool is_batch = false;
  uint64_t N = 0, E = 0, Ebytes = 0, F = 0, seed = 0;
  uint64_t B = 0, P = 1, PS = 0;
  // id -> partition without a 64-bit division on the per-round path: for ids
  // and PartitionSize below 2^32, floor(id * ceil(2^64 / PS) / 2^64) = id / PS
  uint64_t ps_magic = 0;
  uint64_t part_of(uint64_t id) const {
    return ps_magic && id < (1ull << 32) ? (uint64_t)(((unsigned __int128)id * ps_magic) >> 64) : id / PS;
  }
  uint32_t shard = 0, nshards = 1;   // partition p is owned when p % nshards == shard
  bool skipPrep = false;
  // SimpleBatchPianoPIR stats (batch-pir.go:46-52)
  uint64_t FBN = 0, QMIP = 0, Support = 0, prepCount = 0;
  double prepTime = 0, storage = 0, commOn = 0, commOff = 0;

  std::shared_ptr<DevBuf> db = std::make_shared<DevBuf>();   // server DB; shared by the clients of pm_batchpir_create_client
  std::shared_ptr<DevBuf> img = std::make_shared<DevBuf>();  // the DB's fold image (pmk::fold_image), shared likewise
  uint32_t img_npk = 0;   // its packed coordinate slices (FOLD_ROT512P; 0: a plain image), the server's for a client
  uint32_t img_bits = 0;  // its bit-packed fields (FOLD_ROT512Q, pmk::fold_bits_form; then img_npk is 0), the server's for a client
  // the DB's packed row image for the pair answer (pmk::answer_pack_image), shared likewise; its 16-B segments
  // per row (0: no image) and how many of them are coordinates.  step_db puts them into a step.
  std::shared_ptr<DevBuf> apk = std::make_shared<DevBuf>();
  uint32_t apk_nseg = 0, apk_cseg = 0;
  void step_db(PmStep& S) const {
    S.db = db->as<uint64_t>();
    S.dbp = apk_nseg ? apk->as<uint64_t>() : nullptr;
    S.pk_nseg = apk_nseg; S.pk_cseg = apk_cseg;
  }
  DevBuf zero16, parts_d, owned_d, tag, pp, parity, ridx, rval, hist, fqn, arena, tab, tabT, cur, done, gran;
  HostBuf parts_stage;   // pinned copy of [parts | owned parts] for the asynchronous upload (upload_parts_async)
  hipEvent_t stage_ev = nullptr;   // the last upload from parts_stage (the stage is rewritten only after it)
  hipEvent_t order_ev = nullptr;   // upload_parts_async: the client's stream's queued work, waited for on the device
  uint32_t gran_words = 0;
  std::vector<uint32_t> owned_list;   // owned partitions in order (owned_d holds their PmPart)
  DevBuf qoffs, ans_srv;   // the server role's offset sets (then their partitions) and answers, one chunk of a call
  DevBuf srv_parts;        // pm_batchpir_server_answer: [P] PmSrvPart, uploaded by the first call (they never change)
  bool srv_parts_up = false;
  // The client role's split query (pm_batchpir_client_begin / _finish): between the two
  // calls the step's descriptor (its scratch is `buf`, its host view subs / sb / sub_gid / resp_map), the
  // caller's ids and each sub-query's answer row (~0u: it sent no set).  Buffers of its own: qoffs /
  // ans_srv are the server call's, which may run on this handle in between.
  struct SplitQuery {
    bool open = false;
    PmStep S{};
    uint64_t nq = 0;
    std::vector<uint64_t> ids;
    std::vector<uint32_t> map;
    DevBuf sets_d, ans_d, map_d;   // [nsub][qw] sets then [nsub] modes; [nq][E] answers; [nsub] map
    HostBuf sets_h;                // the sets and modes, down
  } split;
  // A client with no DB on the device (pm_batchpir_create_remote): db, img, apk and tab stay
  // empty, and its hints come from streamed preprocessings alone.  prepared: a stream has completed (or
  // DummyPreprocessing ran); prep_due: the re-preprocessing trigger fired in pm_batchpir_client_finish, which
  // cannot preprocess here, and the next begin waits for a stream.
  bool remote = false, prepared = false, prep_due = false;
  // The streamed preprocessing (pm_stream.cpp): which chunks have come, and two pinned staging slots with
  // their device windows, reused round-robin (ev[i]: slot i's last upload and kernels).
  struct PrepStream {
    bool open = false;
    std::vector<std::vector<char>> got;   // [P][SS] chunk delivered
    uint64_t missing = 0;                 // chunks still to come
    HostBuf stage[2];
    DevBuf win[2];
    hipEvent_t ev[2] = {};
    bool busy[2] = {};                    // ev[i] has been recorded
    uint64_t slot_bytes = 0;
    uint32_t next = 0;
    std::chrono::steady_clock::time_point t0;
  } pstream;
  StepBufs buf;   // the step's scratch (engine_step)
  std::vector<double> stamp_sum;   // PM_STAMPS builds: accumulated phase deltas
  uint64_t stamp_n = 0;
  uint32_t step_token = 0;         // PmStep::token of the last step
  uint64_t step_seq = 0;           // its completion sequence number (pm_ctx::record_done)
  size_t pf_off = 0, pf_len = ~size_t(0);   // bytes of each result row the caller reads next
  bool rows_partial = false;   // this call's caller reads ONLY those bytes (GetVertexInfo): the rest is not sent
  HostBuf err_h, src_h;   // src_h: pm_batchpir_query_dev's row pointers
  HostBuf stage_h;                       // ... and its rows of a multi-step query (pinned staging)
  hipEvent_t dev_ev = nullptr;           // ... its completion, for the consumer's stream
  ~Engine() {
    if (dev_ev) (void)hipEventDestroy(dev_ev);
    if (stage_ev) (void)hipEventDestroy(stage_ev);
    if (order_ev) (void)hipEventDestroy(order_ev);
    for (hipEvent_t e : pstream.ev) if (e) (void)hipEventDestroy(e);
  }
  std::vector<PartHost> parts;
  uint32_t maxH = 0, maxPH = 0, maxSS = 0, maxRepl = 0, maxCS = 0, minCS = ~0u;
  bool ph8 = true;   // every owned partition's PH is a multiple of 8 (16-B hint search rows)

  // per-step host view
  std::vector<PmSub> subs;
  std::vector<uint32_t> sb;
  std::vector<uint64_t> sub_gid;   // global id per REAL / HOSTCACHE sub
  PmOutHdr* hdr = nullptr;         // results of the last step (pinned)
  uint64_t* rows = nullptr;
  // batch_query scratch
  std::vector<std::vector<uint64_t>> pq;
  FlatMap resp_map;
  std::vector<uint64_t> resp_rows;
  std::vector<float> resp_dist;
  std::vector<uint8_t> resp_ok;
  std::vector<char> slow;           // partitions at their query budget this batch (bq_prepare)
  uint64_t qn = 0;                  // queryNumToMake of the batch being served
  uint64_t prep_gen = 0;            // preprocessings run (any range): a shared step re-copies the parts
  std::vector<uint64_t> zero_row;   // response of dropped / failed ids (batch-pir.go:229-236)
  // The device loop's copy of the localCache indexes (pm_drl.hip): [P][cmask + 1]
  // entries {local idx + 1 | arena slot << 32}.  cache_on_dev: the device copy
  // is the truth and the host FlatMaps are stale (ensure_host_cache brings them
  // back); dcache_valid: the device copy equals the host's.
  DevBuf dcache;
  uint32_t dcache_cmask = 0;
  bool cache_on_dev = false, dcache_valid = false;
};

// Algorithmic bytes of one answered (real or dummy) sub-query, SURVEY.md §8(d):
// (#in-range rows)*E*8 + 4*SS + 8*E.  A row i*CS + off_i >= N is padding the
// server skips (pir.go:78-84); with uniform offsets the expected number of
// in-range rows is N / CS exactly (every full chunk, plus the partial chunk's
// share), so padding chunks are not counted.
static inline double answer_bytes(const PmPart& d, uint64_t E) {
  const double rows = std::min((double)d.SS, (double)d.N / (double)d.CS);
  return rows * (double)E * 8 + 4.0 * d.SS + 8.0 * E;
}

// A DB generated on the device instead of uploaded: kind 0 = uniform words
// (pm_batchpir_create_synth), kind 1 = the synthetic graph's PIRGraphInfo
// entries (pm_graph_create_synth, graph_synth_elem).
struct DbGen { int kind; uint64_t seed; uint32_t dim, m; };

// the batch PIR handle (pm_pir, which only pm_engine.cpp uses, is beside print_stamps there)
struct pm_batchpir { Engine e; ~pm_batchpir() { print_stamps(e); } };

struct SplitMix {   // host id stream standing in for Go's global math/rand
  uint64_t s;
  uint64_t next() { s += 0x9e3779b97f4a7c15ULL; uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL; z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31); }
  uint64_t intn(uint64_t n) { return next() % n; }
};
struct VD { float dist; int64_t id; };

struct pm_graph {
  pm_ctx* ctx = nullptr;
  uint64_t n = 0, dim = 0, m = 0;
  bool nonprivate = false, skipPrep = false;
  uint64_t pir_seed = 0;
  SplitMix rng{0};
  // host vectors and graph (the success check, non-private mode, DB packing)
  // and their device copy; sessions of one base share them
  std::shared_ptr<const std::vector<float>> vec_own;
  std::shared_ptr<const std::vector<uint32_t>> graph_own;
  const float* vectors = nullptr;
  const uint32_t* graph = nullptr;
  std::shared_ptr<DevBuf> dvec = std::make_shared<DevBuf>();
  std::shared_ptr<DevBuf> dgraph = std::make_shared<DevBuf>();   // [n][m] on the device (device loop), made on first use
  // Sharded / synthetic graphs (pm_graph_create_shard / _synth): the batch
  // PIR holds the partitions p % nshards == shard only, and there is no device
  // copy of all vectors (dvec stays empty): the start set's vectors, fetched
  // non-privately like GetStartVertex (private-search.go:508-531), live in
  // dstartvec.  A synthetic graph has no host arrays either: its rows are
  // graph_synth_elem of data_seed.
  uint32_t shard = 0, nshards = 1;
  bool synth = false;
  uint64_t data_seed = 0;
  DevBuf dstartvec;
  std::vector<uint8_t> okv;            // sharded loop: success flags of a multi-step batch
  const uint32_t* true_nb(uint64_t id, uint32_t* tmp) const {   // the graph's neighbour list of id
    if (!synth) return graph + id * m;
    const uint64_t kg = sm64(data_seed + DOM_SYNTH_NB);
    for (uint32_t k = 0; k < m; ++k) tmp[k] = graph_synth_nb(kg, n, id, (uint32_t)m, k);
    return tmp;
  }
  pm_batchpir* server = nullptr;   // sessions: the base's batch PIR whose server DB they share
  DevBuf dq, dids, ddist;
  float* q_shared = nullptr;   // batched serving: this session's query slot in its group's buffer
  float* qdev() { return q_shared ? q_shared : dq.as<float>(); }
  HostBuf stage_h;                                // pinned: query and start-vertex distances
  pm_batchpir* pir = nullptr;
  std::vector<uint64_t> start;   // StartVertices ids
  DevBuf dstart;
  uint64_t total = 0, succ = 0;
  // SearchKNN scratch, reused across calls (no per-step allocation)
  std::vector<int64_t> batch;
  std::vector<uint64_t> qids;
  std::vector<const uint64_t*> rowp;              // response rows of the last GetVertexInfo
  std::vector<float> dist, start_d;
  std::vector<uint32_t> nb;                       // [len(batch)][m] of the last GetVertexInfo
  FlatMap known;                                  // knownVertices: id -> slot
  std::vector<uint32_t> known_nb;                 // [slot][m]
  std::vector<float> known_dist;
  std::vector<int64_t> known_id, known_reach;
  std::vector<VD> heap, all;
  std::vector<std::pair<VD, uint32_t>> fs;
  Clock::time_point t_init;
  // pm_search_knn_batch's device path: a chunk's queries, answers and
  // empty-heap flags; whether every id of the graph is < n (-1: not checked yet)
  DevBuf kb_q, kb_ids, kb_steps, kb_flags;
  int graph_ids_ok = -1;
  // A device-loop call that failed after queueing work (run_batched_dev) leaves
  // the session's host mirrors (FinishedBatchNum, QueriesMadeInPartition, the
  // search and dummy streams) out of step with its device state; the session
  // is then unusable and every later call on it fails with this reason.
  std::string lost;
  ~pm_graph() { delete pir; }
};

struct ShardComb;
struct StepGroup {
  pm_ctx* c = nullptr;   // the shared steps' stream
  uint32_t S = 0, P = 0, maxPH = 0, maxSS = 0, E = 0, dim = 0;
  // the partitions the clients hold (all P, or a shard's p % nshards == shard);
  // client s's partition lp[i] is the shared step's partition s * Pl + i
  std::vector<uint32_t> lp;
  uint32_t Pl = 0;
  bool ph8 = false;
  // the shared step's scratch (group_step).  The device loop sizes it once
  // (drl_team_init) and its kernels keep the pointers: no group_step, nor any
  // other reserve of it, on a DrlTeam's group after that
  StepBufs buf;
  DevBuf parts_d, done, prep_parts, desc_d;
  uint32_t token = 0, pf_w0 = 0, pf_w1 = 0;
  uint64_t seq = 0;   // the last shared step's completion sequence number (pm_ctx::record_done)
  std::vector<PmSub> subs;
  std::vector<uint32_t> sb, base;
  uint32_t nsub = 0;           // the last shared step's sub-queries
  // Descriptor staging (pooled serving, group_stage_session): each session's
  // task writes its next sub-queries into its own slot of stage_h (stride
  // PmSubs each), so the launching worker only compacts the slots instead of
  // reading every session's sub-queries out of other cores' caches.
  struct alignas(64) SessStage {
    uint64_t step = ~0ull;   // the shared step (G.nstep) the slot was written for
    uint32_t n = 0, nreal = 0, maxpp = 0, live = 0;
    double bytes = 0;
    bool ok = false;
    std::vector<uint32_t> pc;   // [Pl] sub-queries per partition
  };
  bool stage_on = false;
  uint32_t stride = 0;
  uint64_t nstep = 0;
  HostBuf stage_h;
  std::vector<SessStage> stg;
  std::vector<uint64_t> gen;   // each session's Engine::prep_gen at the last upload of its parts
  std::vector<Engine*> es;     // the clients (batch PIR engines) sharing the steps
  std::vector<const float*> qv;   // each client's search query on the device (null: no distances)
  bool rows_partial = false;   // graph search: only the neighbour words of each row go to the host
  // the sessions' queries and start sets, scored in ONE k_l2_rows launch per query
  uint32_t ns = 0;
  DevBuf qbuf, start_ids, start_dist, start_vec;   // start_vec: [S][ns][dim] (sharded / synthetic graphs)
  HostBuf qstage;   // [S][dim] queries, then [S][ns] start-set distances
  // ---- sharded private search (pm_search_loop_sharded): this rank's share of
  // every shared step becomes per-id records [S][npos][W] (group_exchange),
  // summed over the ranks by the combine, then read back by every rank
  ShardComb* comb = nullptr;
  uint32_t team = 0;
  uint64_t round = 0;
  std::vector<pm_graph*> gs;
  uint32_t npos = 0, W = 0, w0 = 0, nb_off = 0;   // ids per session per round, record words, first row word
  DevBuf out_d, map_d, ids_d, rec_own;            // step outputs (device), map, ids; the records if not the caller's
  uint64_t* rec_d = nullptr;                      // [S*npos*W] records + 1 error word (all-reduced)
  std::atomic<bool> peer_failed{false};           // a combine's error word was nonzero: no further turns
  uint32_t verify_every = 0;                      // pm_set_option("verify_records") at the loop's start
  bool combine_dead = false;                      // the collective itself failed / timed out: no further turns
  DevBuf st_d;                                    // ... the status words when the records are the caller's buffer
  HostBuf map_h, ids_h, slow_h, rec_h;
  std::vector<char> slow;                         // sessions served by the multi-step path this round
};

struct StreamSwap {   // a team context's stream replaced for the loop's duration (restored drained)
  pm_ctx* c = nullptr;
  hipStream_t old = nullptr;
  void swap_in(pm_ctx* ctx, hipStream_t st) {
    if (!st) return;
    c = ctx; old = ctx->stream;
    (void)hipStreamSynchronize(old);
    ctx->stream = st;
  }
  ~StreamSwap() {
    if (!c) return;
    (void)hipStreamSynchronize(c->stream);
    c->stream = old;
  }
};
