// pm_engine.cpp — host side of libpacmann.so: the PianoPIR / SimpleBatchPianoPIR
// engine (device-resident DB, hints and client state; batched steps), the
// graphann beam search over PIRGraphInfo, and the extern "C" boundary of
// include/pacmann.h.
#include "pm_host.h"

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

static void derive_key(uint64_t seed, uint64_t part, uint64_t epoch, uint8_t key[16]) {
  uint64_t r1 = hash4(seed, DOM_KEY, part, epoch, 0), r2 = hash4(seed, DOM_KEY, part, epoch, 1);
  memcpy(key, &r1, 8);
  memcpy(key + 8, &r2, 8);
}

// ---------------------------------------------------------------------------
// One step's scratch (k_match -> k_resolve -> [k_gather] -> k_answer), held by
// an Engine for its own steps and by a StepGroup for its shared ones.  The
// device buffers are sized by reserve() for nsub sub-queries over np
// partitions; part_x (split gather), stamps (stamp builds) and the pinned
// descriptor / result buffers are reserved where a step needs them.
// ---------------------------------------------------------------------------
struct StepBufs {
  DevBuf subs_d, sb_d, bits, cand, meta, spec, res_d, ans, part_x, stamps;
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
  DevBuf zero16, parts_d, owned_d, tag, pp, parity, ridx, rval, hist, fqn, arena, tab, tabT, cur, done, gran;
  HostBuf parts_stage;   // pinned copy of [parts | owned parts] for the asynchronous upload (upload_parts_async)
  hipEvent_t stage_ev = nullptr;   // the last upload from parts_stage (the stage is rewritten only after it)
  hipEvent_t order_ev = nullptr;   // upload_parts_async: the client's stream's queued work, waited for on the device
  uint32_t gran_words = 0;
  std::vector<uint32_t> owned_list;   // owned partitions in order (owned_d holds their PmPart)
  DevBuf qoffs, ans_srv;
  StepBufs buf;   // the step's scratch (engine_step)
  DevBuf helpg;   // k_step's gather helpers' hand-off granules
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

// NewPianoPIR parameterisation (pir.go:479-514) + NewPianoPIRClient (:130-175)
static void part_params(PartHost& ph, uint64_t N, uint64_t F) {
  uint64_t target = (uint64_t)(2 * std::sqrt((double)N));
  uint64_t cs = 1;
  while (cs < target) cs *= 2;
  uint64_t ss = (uint64_t)std::ceil((double)N / (double)cs);
  ss = (ss + 3) / 4 * 4;
  const uint64_t thr = 8;   // PianoPIRConfig.ThreadNum (pir.go:502)
  uint64_t maxq = (uint64_t)(std::sqrt((double)N) * std::log((double)N));
  uint64_t k = (uint64_t)std::ceil(std::log(2.0) * (double)(F + 1));
  uint64_t phn = (k * cs + thr - 1) / thr * thr;
  uint64_t qpc = 3 * (uint64_t)((double)maxq / (double)ss);
  qpc = (qpc + thr - 1) / thr * thr;
  ph.d.N = N;
  ph.d.CS = (uint32_t)cs;
  uint32_t lg = 0; while ((1ull << lg) < cs) ++lg;
  ph.d.log2CS = lg;
  ph.d.SS = (uint32_t)ss;
  ph.d.PH = (uint32_t)phn;
  ph.d.Qpc = (uint32_t)qpc;
  ph.d.H = (uint32_t)(phn + ss * qpc);
  ph.maxq64 = maxq;
  ph.d.MaxQ = (uint32_t)std::min<uint64_t>(maxq, 0xffffffffu);
}

static double part_storage(const PartHost& p, uint64_t Ebytes) {   // LocalStorageSize pir.go:178-190
  double s = 0;
  s = s + (double)p.d.PH * 8;
  s = s + (double)p.d.PH * (double)Ebytes;
  s = s + (double)p.d.PH * 8;
  double tb = (double)p.d.SS * (double)p.d.Qpc;
  s = s + tb * 8;
  s = s + tb * (double)Ebytes;
  s = s + tb * 8;
  s = s + tb * (double)Ebytes;
  return s;
}
static double part_comm(const PartHost& p, uint64_t E) { return (double)((uint64_t)p.d.SS * 4 + E * 8); }
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
static int engine_create(pm_ctx* ctx, Engine* g, uint64_t N, uint64_t Ebytes, uint64_t B,
                         const uint64_t* rawDB, uint64_t F, uint64_t seed, bool batch,
                         uint32_t shard = 0, uint32_t nshards = 1, const Engine* server = nullptr,
                         const DbGen* gen = nullptr) {
  if (nshards == 0 || shard >= nshards) return fail(PM_EINVAL, "shard must be < nshards");
  if (!ctx) return fail(PM_EINVAL, "ctx is NULL");
  if (!rawDB && N && !server && !gen) return fail(PM_EINVAL, "rawDB is NULL");
  if (gen && gen->kind == 1 && (uint64_t)(gen->dim + gen->m) * 4 != Ebytes)
    return fail(PM_EINVAL, "graph entry size must be 4 * (dim + m)");
  if (server && server->ctx->device != ctx->device) return fail(PM_EINVAL, "a client shares the server DB of its own device only");
  if (N == 0) return fail(PM_EINVAL, "DBSize must be > 0");
  if (Ebytes < 8) return fail(PM_EINVAL, "DBEntryByteNum must be >= 8");
  HIPCHK(hipSetDevice(ctx->device));
  g->ctx = ctx; g->is_batch = batch;
  g->N = N; g->Ebytes = Ebytes; g->E = Ebytes / 8; g->F = F; g->seed = seed;
  if (batch) {
    g->B = B;
    g->P = B / 2;   // BatchSize / RealQueryPerPartition (batch-pir.go:62)
    if (g->P == 0) return fail(PM_EINVAL, "BatchSize must be >= 2");
    g->PS = (N + g->P - 1) / g->P;
    if (g->PS > 1 && g->PS < (1ull << 32)) g->ps_magic = ~0ull / g->PS + 1;
  } else {
    g->P = 1; g->PS = N;
  }
  g->parts.resize(g->P);
  if (g->E > pmk::step_max_e()) return fail(PM_EINVAL, "DBEntrySize above the step kernel's LDS limit");
  g->shard = shard; g->nshards = nshards;
  uint64_t off_tag = 0, off_pp = 0, off_par = 0, off_ridx = 0, off_rval = 0, off_hist = 0, off_ar = 0,
           off_tab = 0, off_tabT = 0, off_cur = 0, off_db = 0;
  for (uint64_t i = 0; i < g->P; ++i) {
    PartHost& ph = g->parts[i];
    uint64_t start = i * g->PS, end = std::min((i + 1) * g->PS, N);
    if (end <= start) return fail(PM_EINVAL, "empty partition (DBSize too small for BatchSize)");
    part_params(ph, end - start, F);
    ph.owned = i % nshards == shard;
    if (!ph.owned) {   // parameters only (bucketing and accounting are global)
      ph.d.seed = seed; ph.d.idx = i;
      continue;
    }
    g->owned_list.push_back((uint32_t)i);
    if (ph.d.CS > 32768) return fail(PM_EINVAL, "ChunkSize > 32768 unsupported (16-bit prep offsets)");
    if (ph.d.SS > pmk::step_max_ss()) return fail(PM_EINVAL, "SetSize above the step kernel's LDS limit");
    if ((uint64_t)ph.d.H >= (1ull << 29)) return fail(PM_EINVAL, "tag space >= 2^29 (util.go:161)");
    ph.d.row0 = off_db; off_db += end - start;   // rows of owned partitions, packed
    ph.d.seed = seed; ph.d.idx = i;
    g->maxH = std::max(g->maxH, ph.d.H);
    g->maxCS = std::max(g->maxCS, ph.d.CS);
    g->minCS = std::min(g->minCS, ph.d.CS);
    g->maxPH = std::max(g->maxPH, ph.d.PH);
    g->ph8 = g->ph8 && ph.d.PH % 8 == 0;
    g->maxSS = std::max(g->maxSS, ph.d.SS);
    g->maxRepl = std::max(g->maxRepl, ph.d.SS * ph.d.Qpc);
    // carve offsets (elements)
    ph.d.tag = (uint32_t*)(uintptr_t)off_tag; off_tag += ph.d.H;
    ph.d.pp = (uint32_t*)(uintptr_t)off_pp; off_pp += ph.d.PH;
    ph.d.parity = (uint64_t*)(uintptr_t)off_par; off_par += (uint64_t)ph.d.H * g->E;
    ph.d.ridx = (uint32_t*)(uintptr_t)off_ridx; off_ridx += (uint64_t)ph.d.SS * ph.d.Qpc;
    ph.d.rval = (uint64_t*)(uintptr_t)off_rval; off_rval += (uint64_t)ph.d.SS * ph.d.Qpc * g->E;
    ph.d.hist = (uint32_t*)(uintptr_t)off_hist; off_hist += ph.d.SS;
    ph.d.arena = (uint64_t*)(uintptr_t)off_ar; off_ar += (uint64_t)ph.d.MaxQ * g->E;
    ph.d.tab = (uint16_t*)(uintptr_t)off_tab; off_tab += (uint64_t)ph.d.H * ph.d.SS;
    ph.d.curk = cur_k(ph.d.PH, ph.d.SS);
    ph.d.cur = (uint16_t*)(uintptr_t)off_cur; off_cur += cur_words(ph.d.PH, ph.d.SS, ph.d.curk);
    ph.d.tabT = (uint16_t*)(uintptr_t)off_tabT; off_tabT += tabT_words(ph.d.H, ph.d.SS);
    ph.cache.reserve(ph.d.MaxQ);
  }
  CHK(g->zero16.reserve(64));
  HIPCHK(hipMemset(g->zero16.p, 0, 64));
  if (server) g->db = server->db;   // same N, entry size, partitions and shard: same packed rows
  else CHK(g->db->reserve(std::max<uint64_t>(8, off_db * g->E * 8)));
  for (uint32_t i : server ? std::vector<uint32_t>{} : g->owned_list) {
    const uint64_t start = (uint64_t)i * g->PS, rows = g->parts[i].d.N;
    uint64_t* dst = g->db->as<uint64_t>() + g->parts[i].d.row0 * g->E;
    if (gen && gen->kind == 0)
      pmk::db_synth(ctx->stream, dst, start, rows, (uint32_t)g->E, gen->seed);
    else if (gen)
      pmk::graph_synth(ctx->stream, dst, start, rows, N, gen->dim, gen->m, gen->seed);
    else
      HIPCHK(hipMemcpy(dst, rawDB + start * g->E, rows * g->E * 8, hipMemcpyHostToDevice));
  }
  if (gen) {
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  // the fold image: a second copy of the owned partitions' rows, laid out for
  // k_prep_fold_rot (CS 512 and 1,024 shapes; PM_FOLD_ROT=0 disables it).  It is
  // skipped, and the fold reads the rows themselves (k_prep_fold_pipe), when
  // it would take more than a quarter of the device memory still free.
  uint64_t off_img = 0;
  if (!g->owned_list.empty() && pmk::fold_image_ok(g->minCS, g->maxCS, (uint32_t)g->E)) {
    for (uint32_t i : g->owned_list) {
      PmPart& d = g->parts[i].d;
      d.img = (const uint64_t*)(uintptr_t)off_img;
      off_img += pmk::fold_image_words(d.SS, (uint32_t)g->E, (uint32_t)g->maxCS);
    }
    size_t free_b = 0, total_b = 0;
    if (!server && hipMemGetInfo(&free_b, &total_b) == hipSuccess && off_img * 8 > free_b / 4) {
      for (uint32_t i : g->owned_list) g->parts[i].d.img = nullptr;
      off_img = 0;
    } else if (server && !server->img->p) {   // the server went without one
      for (uint32_t i : g->owned_list) g->parts[i].d.img = nullptr;
      off_img = 0;
    }
  }
  if (off_img) {
    if (server) {
      g->img = server->img;
    } else {
      CHK(g->img->reserve(off_img * 8));
      for (uint32_t i : g->owned_list) {
        const PmPart& d = g->parts[i].d;
        pmk::fold_image(ctx->stream, g->img->as<uint64_t>() + (uintptr_t)d.img, g->db->as<uint64_t>() + d.row0 * g->E,
                        d.N, d.SS, (uint32_t)g->E, (uint32_t)g->maxCS);
      }
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(ctx->stream));
    }
  }
  CHK(g->tag.reserve(off_tag * 4));
  CHK(g->pp.reserve(off_pp * 4));
  CHK(g->parity.reserve(off_par * 8));
  CHK(g->ridx.reserve(off_ridx * 4));
  CHK(g->rval.reserve(off_rval * 8));
  CHK(g->hist.reserve(off_hist * 4));
  CHK(g->fqn.reserve(g->P * 4));
  CHK(g->arena.reserve(std::max<uint64_t>(8, off_ar * 8)));
  // the chunk-major PRF table only where the fold reads it (every other reader uses tabT):
  // SIFT1M's rotated fold and the BIGANN wide fold do not, saving H*SS*2 B per partition
  const bool need_tab = pmk::fold_needs_tab(g->minCS, g->maxCS, (uint32_t)g->E, off_img != 0);
  if (need_tab) CHK(g->tab.reserve(off_tab * 2));
  CHK(g->tabT.reserve(off_tabT * 2));
  CHK(g->cur.reserve(std::max<uint64_t>(2, off_cur * 2)));
  CHK(g->done.reserve(4 * (3 + 16 * 4096)));
  {   // step completion counter (pm_query.hip chain_add): 2^31 in the low half, 0 chained
    const uint32_t init[3] = {1u << 31, 0, 0};
    HIPCHK(hipMemcpy(g->done.p, init, sizeof init, hipMemcpyHostToDevice));
  }
  {   // k_step hand-off granules (token 0 never marks a step) and the error word
    g->gran_words = (g->maxPH + 63) / 64;
    const size_t n = (size_t)kArgSubs * (8 + 64 + 2 * g->gran_words + 8) * 8;
    CHK(g->gran.reserve(n));
    HIPCHK(hipMemset(g->gran.p, 0, n));
    CHK(g->err_h.reserve(64));
    memset(g->err_h.p, 0, 64);
  }
  CHK(g->parts_d.reserve(g->P * sizeof(PmPart)));
  CHK(g->owned_d.reserve(std::max<size_t>(1, g->owned_list.size()) * sizeof(PmPart)));
  CHK(g->parts_stage.reserve((g->P + g->owned_list.size()) * sizeof(PmPart)));
  for (uint64_t i = 0; i < g->P; ++i) {
    PmPart& d = g->parts[i].d;
    if (!g->parts[i].owned) continue;
    d.tag = g->tag.as<uint32_t>() + (uintptr_t)d.tag;
    d.pp = g->pp.as<uint32_t>() + (uintptr_t)d.pp;
    d.parity = g->parity.as<uint64_t>() + (uintptr_t)d.parity;
    d.ridx = g->ridx.as<uint32_t>() + (uintptr_t)d.ridx;
    d.rval = g->rval.as<uint64_t>() + (uintptr_t)d.rval;
    d.hist = g->hist.as<uint32_t>() + (uintptr_t)d.hist;
    d.fqn = g->fqn.as<uint32_t>() + i;
    d.arena = g->arena.as<uint64_t>() + (uintptr_t)d.arena;
    d.tabT = g->tabT.as<uint16_t>() + (uintptr_t)d.tabT;
    d.tab = need_tab ? g->tab.as<uint16_t>() + (uintptr_t)d.tab : nullptr;
    d.cur = g->cur.as<uint16_t>() + (uintptr_t)d.cur;
    d.img = off_img ? g->img->as<uint64_t>() + (uintptr_t)d.img : nullptr;
  }
  HIPCHK(hipMemsetAsync(g->fqn.p, 0, g->P * 4, ctx->stream));
  HIPCHK(hipMemsetAsync(g->hist.p, 0, off_hist * 4, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return 0;
}

static int upload_parts(Engine* g) {
  std::vector<PmPart> v(g->P), w;
  for (uint64_t i = 0; i < g->P; ++i) v[i] = g->parts[i].d;
  for (uint32_t i : g->owned_list) w.push_back(g->parts[i].d);
  HIPCHK(hipMemcpyAsync(g->parts_d.p, v.data(), g->P * sizeof(PmPart), hipMemcpyHostToDevice,
                        g->ctx->stream));
  if (!w.empty())
    HIPCHK(hipMemcpyAsync(g->owned_d.p, w.data(), w.size() * sizeof(PmPart), hipMemcpyHostToDevice,
                          g->ctx->stream));
  HIPCHK(hipStreamSynchronize(g->ctx->stream));   // v, w go out of scope
  return 0;
}

// upload_parts without the host round trip: the parts staged in pinned memory
// and copied on `st` (a multi-client maintenance enqueues every client's copy
// on its launch stream and synchronises once, after the preprocessing
// kernels; one pageable copy + synchronisation per client cost ~80 us each,
// 21 ms for 256 SIFT1M clients).  The stage is rewritten only by this
// client's next preprocessing, after that synchronisation.
static int upload_parts_async(Engine* g, hipStream_t st) {
  // the parts are read by kernels on the client's own stream too: anything still
  // queued there finishes before the copy overwrites them.  Ordered on the
  // device (an event the copy's stream waits for), not by a host wait: in the
  // device loop a team leader's stream is busy with the query just queued, and
  // a host synchronisation there stalled the next teams' enqueueing
  if (g->ctx->stream != st && hipStreamQuery(g->ctx->stream) != hipSuccess) {
    if (!g->order_ev) HIPCHK(hipEventCreateWithFlags(&g->order_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(g->order_ev, g->ctx->stream));
    HIPCHK(hipStreamWaitEvent(st, g->order_ev, 0));
  }
  const size_t no = g->owned_list.size();
  if (g->stage_ev) HIPCHK(hipEventSynchronize(g->stage_ev));   // the previous upload has left the stage
  else HIPCHK(hipEventCreateWithFlags(&g->stage_ev, hipEventDisableTiming));
  CHK(g->parts_stage.reserve((g->P + no) * sizeof(PmPart)));
  PmPart* h = g->parts_stage.as<PmPart>();
  for (uint64_t i = 0; i < g->P; ++i) h[i] = g->parts[i].d;
  for (size_t i = 0; i < no; ++i) h[g->P + i] = g->parts[g->owned_list[i]].d;
  HIPCHK(hipMemcpyAsync(g->parts_d.p, h, g->P * sizeof(PmPart), hipMemcpyHostToDevice, st));
  if (no) HIPCHK(hipMemcpyAsync(g->owned_d.p, h + g->P, no * sizeof(PmPart), hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(g->stage_ev, st));
  return 0;
}

// Client.Preprocessing (pir.go:267-301) for partitions [p0, p1): Initialization
// (new key, reset state) then, unless skipPrep, the full hint fold.
// Client.Initialization's host side for the owned partitions in [p0, p1)
// (pir.go:203-255: new key from the next epoch, reset counters and cache);
// uploads the parts (on `st` without synchronising when given).  Fills `todo`
// with the partitions to fold.
// The localCache indexes back from the device loop's copy (pm_drl.hip) before
// a host-side use: the FlatMaps are rebuilt from the device table, which is
// then stale (the host path owns the index until the next device loop).
// Callers have synchronised the loop's streams (it ends with them drained).
static int ensure_host_cache(Engine* g) {
  if (!g->cache_on_dev) return 0;
  const uint64_t cap = (uint64_t)g->dcache_cmask + 1;
  std::vector<uint64_t> t(g->P * cap);
  HIPCHK(hipSetDevice(g->ctx->device));
  HIPCHK(hipMemcpy(t.data(), g->dcache.p, t.size() * 8, hipMemcpyDeviceToHost));
  for (uint64_t p = 0; p < g->P; ++p) {
    FlatMap& c = g->parts[p].cache;
    c.clear();
    for (uint64_t i = 0; i < cap; ++i)
      if (const uint64_t e = t[p * cap + i]) c.put((uint32_t)e - 1u, (uint32_t)(e >> 32));
  }
  g->cache_on_dev = false;
  g->dcache_valid = false;
  return 0;
}

static int engine_prep_host(Engine* g, uint64_t p0, uint64_t p1, std::vector<uint64_t>& todo,
                            hipStream_t st = nullptr) {
  // the owned partitions in [p0, p1): all of them (owned_d) or a single one
  if (p1 - p0 > 1 && !(p0 == 0 && p1 == g->P)) return fail(PM_EINVAL, "engine_prep: unsupported range");
  const bool all = p0 == 0 && p1 == g->P;
  if (g->cache_on_dev && !all) CHK(ensure_host_cache(g));   // one partition's prep keeps the others' entries
  if (all) { g->cache_on_dev = false; g->dcache_valid = false; }   // every index cleared below: the host's (empty) is the truth
  todo.clear();
  for (uint64_t i = p0; i < p1; ++i)
    if (g->parts[i].owned) todo.push_back(i);
  if (todo.empty()) return 0;
  for (uint64_t i : todo) {
    PartHost& ph = g->parts[i];
    uint8_t key[16];
    derive_key(g->seed, i, ph.epoch_ctr, key);
    ph.d.epoch = ph.epoch_ctr++;
    pm_expand_key(key, ph.d.rk);
    ph.fqn = 0;
    ph.cache.clear();
    ph.shadow.clear();
  }
  CHK(st ? upload_parts_async(g, st) : upload_parts(g));
  g->prep_gen++;
  return 0;
}
// The device side for np parts at dp (of one engine, or of several clients of
// one server: same parameters and DB): PRF tables, then the hint fold and
// the replacement rows, or zero hints for DummyPreprocessing.  Synchronous.
static int engine_prep_launch(pm_ctx* c, const Engine* g, const PmPart* dp, int np, const PmPart* host_parts,
                              uint32_t clients = 1, bool sync = true) {
  hipStream_t st = c->stream;
  c->timed("prep_init", 0, [&] { pmk::prep_init(st, dp, np, g->maxH, g->maxRepl, (uint32_t)g->E, g->skipPrep); });
  double aes = 0, fold = 0, repl = 0;
  uint32_t minH = ~0u;
  for (int i = 0; i < np; ++i) {
    const PmPart& d = host_parts[i];
    minH = std::min(minH, d.H);
    aes += (double)d.H * d.SS;
    // algorithmic fold bytes: hpc * SS (hint, chunk) pairs of one E-word entry
    fold += ((double)d.PH + (double)(d.SS - 1) * d.Qpc) * d.SS * (double)g->E * 8;
    repl += (double)d.SS * d.Qpc * g->E * 8 * 2;
  }
  // the replacement rows beside the PRF tables (after prep_init, which they follow on st)
  const bool side = !g->skipPrep && c->repl_side && !c->timing && !c->debug_sync;
  std::unique_lock<std::mutex> side_lk(c->side_mu, std::defer_lock);
  if (side) {
    side_lk.lock();
    if (!c->side) {
      HIPCHK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
      for (auto& e : c->side_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    HIPCHK(hipEventRecord(c->side_ev[0], st));
    HIPCHK(hipStreamWaitEvent(c->side, c->side_ev[0], 0));
    pmk::prep_repl(c->side, dp, np, g->maxRepl, g->db->as<uint64_t>(), (uint32_t)g->E);
    HIPCHK(hipEventRecord(c->side_ev[1], c->side));
  }
  // the PRF table is built even by DummyPreprocessing: queries still evaluate the PRF
  c->timed("prep_offsets", aes, [&] { pmk::prep_offsets(st, dp, np, g->maxH, g->maxSS); });
  if (g->skipPrep) {   // DummyPreprocessing (pir.go:520-523): zero hints
    for (int i = 0; i < np; ++i) {
      const PmPart& d = host_parts[i];
      HIPCHK(hipMemsetAsync(d.parity, 0, (uint64_t)d.H * g->E * 8, st));
      HIPCHK(hipMemsetAsync(d.rval, 0, (uint64_t)d.SS * d.Qpc * g->E * 8, st));
    }
  } else {
    int kind = pmk::FOLD_OTHER;
    c->timed("prep_fold", fold, [&] { kind = pmk::prep_fold(st, dp, np, g->maxH, g->db->as<uint64_t>(), (uint32_t)g->E, g->minCS,
                                                      g->maxCS, g->zero16.as<uint64_t>(), clients, g->img->p != nullptr, minH); });
    c->host_add(kind == pmk::FOLD_ROT512 ? HT_FOLD_ROT512 : kind == pmk::FOLD_ROT1024 ? HT_FOLD_ROT1024 : HT_FOLD_OTHER, 0.0);
    if (side) HIPCHK(hipStreamWaitEvent(st, c->side_ev[1], 0));
    else c->timed("prep_repl", repl, [&] { pmk::prep_repl(st, dp, np, g->maxRepl, g->db->as<uint64_t>(), (uint32_t)g->E); });
  }
  HIPCHK(hipGetLastError());
  if (sync) HIPCHK(hipStreamSynchronize(st));
  return 0;
}
static int engine_prep(Engine* g, uint64_t p0, uint64_t p1) {
  std::vector<uint64_t> todo;
  CHK(engine_prep_host(g, p0, p1, todo));
  if (todo.empty()) return 0;
  const PmPart* dp = p1 - p0 == 1 ? g->parts_d.as<PmPart>() + p0 : g->owned_d.as<PmPart>();
  std::vector<PmPart> hp;
  for (uint64_t i : todo) hp.push_back(g->parts[i].d);
  return engine_prep_launch(g->ctx, g, dp, (int)todo.size(), hp.data());
}

// One batched step over the sub-queries in g->subs (partition-major, ranges in
// g->sb): k_match -> k_resolve -> k_answer.  The descriptor is
// read zero-copy from pinned host memory and the results (status header +
// entry + L2 distance to q) are written by the GPU straight into pinned host
// memory, so a step costs three launches and one stream synchronisation.

// Completion of a step.  Every result header in pinned memory carries this
// step's token; the host polls the tokens (and prefetches the bytes [pf_off,
// pf_off + pf_len) of each published row, so the caller's reads hit the cache).
// A token says that its sub-query is answered, not that the row's bytes have
// landed: stores from the GPU to fine-grained host memory reach the host in no
// guaranteed order.  The results are therefore taken only after the step's
// completion event (recorded after its last kernel with a system-scope
// release, pm_ctx::done_ring) is seen complete: from then on every byte the
// step wrote is visible (HIP event semantics).  Rows are then checked against
// their header hash (PmOutHdr::csum) as an assertion: a mismatch is an error,
// never retried.  `torn` counts rows whose bytes did not yet match at token
// time (rows_check >= 1, diagnostics only).
// PM_PUBLISH_WAIT=0 drops the completion wait: rows are then accepted on the
// token and a matching hash, re-read until they match (rows_check 2).
// Debug runs (PM_DEBUG_SYNC), and a step not published within 5 s (a fault, or
// a bug), fall back to the stream synchronisation, which reports errors.
// sc: the context whose stream ran the step (its done_ring); c: the one whose
// counters are charged (a session of a shared step, or sc itself).
static int wait_done(pm_ctx* sc, uint64_t seq) {
  if (sc->done_seen.load(std::memory_order_acquire) >= seq) return 0;
  auto t0 = Clock::now();
  for (uint64_t spin = 0;; ++spin) {
    if (sc->done_seen.load(std::memory_order_acquire) >= seq) return 0;
    if (sc->done_mu.try_lock()) {   // one waiter asks the runtime; the others read done_seen
      std::lock_guard<std::mutex> lk(sc->done_mu, std::adopt_lock);
      if (sc->done_seen.load(std::memory_order_acquire) >= seq) return 0;
      const uint64_t rec = seq;   // this step's own event (done_ring)
      if (sc->done_rec.load(std::memory_order_acquire) < seq)
        return fail(PM_EHIP, "step completion: waited for a step that was not recorded");
      for (uint64_t k = 0;; ++k) {
        const hipError_t e = hipEventQuery(sc->done_ring[seq % pm_ctx::kDoneRing]);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) return fail(PM_EHIP, std::string("step completion: ") + hipGetErrorString(e));
        if ((k & 0xfff) == 0xfff && ms_since(t0) > 5000.0) {
          HIPCHK(hipStreamSynchronize(sc->stream));
          HIPCHK(hipGetLastError());
          break;
        }
      }
      uint64_t prev = sc->done_seen.load(std::memory_order_relaxed);
      while (prev < rec && !sc->done_seen.compare_exchange_weak(prev, rec, std::memory_order_release)) {}
      return 0;
    }
    if ((spin & 0xffff) == 0xffff && ms_since(t0) > 10000.0) return fail(PM_EHIP, "step completion wait timed out");
  }
}

// Non-blocking form of wait_done: *ready once step `seq` of sc's stream has
// completed (its done_ring event), or at once where steps are not ordered by
// their completion event (PM_PUBLISH_WAIT=0: the results' tokens decide).
static int poll_done(pm_ctx* sc, uint64_t seq, bool* ready) {
  *ready = !(sc->publish_wait && sc->done_ev && seq) || sc->done_seen.load(std::memory_order_acquire) >= seq;
  if (*ready || !sc->done_mu.try_lock()) return 0;
  std::lock_guard<std::mutex> lk(sc->done_mu, std::adopt_lock);
  if (sc->done_seen.load(std::memory_order_acquire) >= seq) { *ready = true; return 0; }
  if (sc->done_rec.load(std::memory_order_acquire) < seq)
    return fail(PM_EHIP, "step completion: polled a step that was not recorded");
  const hipError_t e = hipEventQuery(sc->done_ring[seq % pm_ctx::kDoneRing]);
  if (e == hipErrorNotReady) return 0;
  if (e != hipSuccess) return fail(PM_EHIP, std::string("step completion: ") + hipGetErrorString(e));
  uint64_t prev = sc->done_seen.load(std::memory_order_relaxed);
  while (prev < seq && !sc->done_seen.compare_exchange_weak(prev, seq, std::memory_order_release)) {}
  *ready = true;
  return 0;
}

static int wait_step(pm_ctx* c, const PmOutHdr* hdr, uint32_t nsub, uint32_t token, const char* rows,
                     size_t row_bytes, size_t pf_off, size_t pf_len, uint64_t seq, pm_ctx* sc = nullptr) {
  if (!sc) sc = c;
  hipStream_t stream = sc->stream;
  const bool ordered = sc->publish_wait && sc->done_ev && seq;
  const size_t w0 = pf_off / 8, w1 = (pf_off + pf_len + 7) / 8;
  auto row_hash = [&](uint32_t s) {
    const volatile uint64_t* rw = (const volatile uint64_t*)(rows + s * row_bytes);
    uint64_t x = token * kCsumMix;
    for (size_t w = w0; w < w1; ++w) x += rw[w] * c->hash_mult[w];
    return x;
  };
  if (c->debug_sync) {
    HIPCHK(hipStreamSynchronize(stream));
  } else if (ordered && !c->timing) {
    // the results are taken after the step's completion event anyway: wait for
    // it first, then ONE pass over the tokens and row hashes below (the serving
    // loop opens a team's phase only once the event has completed, so this is
    // no wait at all there)
    for (uint32_t s = 0; s < nsub; ++s) {
      __builtin_prefetch(&hdr[s]);
      if (c->rows_check)
        for (size_t w = w0; w < w1; w += 8) __builtin_prefetch(rows + s * row_bytes + w * 8);
    }
    CHK(wait_done(sc, seq));
    std::atomic_thread_fence(std::memory_order_acquire);
  } else {
    const volatile uint32_t* tok = &hdr[0].token;
    const size_t stride = sizeof(PmOutHdr) / sizeof(uint32_t);
    // the headers and checked row words are GPU-written pinned memory (cache
    // misses): all their lines requested at once, not one miss after another
    for (uint32_t s = 0; s < nsub; ++s) {
      __builtin_prefetch(&hdr[s]);
      if (c->rows_check)
        for (size_t w = w0; w < w1; w += 8) __builtin_prefetch(rows + s * row_bytes + w * 8);
    }
    auto t0 = Clock::now();
    uint32_t s = 0;
    bool first_look = true;   // the first read of sub-query s's row after its token appeared
    for (uint64_t spin = 0; s < nsub; ++spin) {
      if (tok[s * stride] == token) {
        if (c->timing && s == 0 && first_look) c->host_add(HT_WAIT_FIRST, ms_since(t0));
        std::atomic_thread_fence(std::memory_order_acquire);
        if (c->rows_check) {
          const bool match = row_hash(s) == *(const volatile uint64_t*)&hdr[s].csum;
          if (first_look) {
            c->host_add(HT_ROWS_SEEN, 0);
            if (!match) c->host_add(HT_ROWS_TORN, 0);
          }
          if (!match && !ordered) {   // token-time acceptance: wait for the bytes to match
            first_look = false;
            if (c->rows_check == 1)
              return fail(PM_EHIP, "step result row " + std::to_string(s) + " does not match its header checksum");
            if ((spin & 0xffff) == 0xffff && ms_since(t0) > 5000.0)
              return fail(PM_EHIP, "step results incomplete (sub-query " + std::to_string(s) + ")");
            continue;
          }
        }
        if (c->timing && s + 1 == nsub) c->host_add(HT_WAIT_ALL, ms_since(t0));
        ++s;
        first_look = true;
        continue;
      }
      if ((spin & 0xffff) == 0xffff && ms_since(t0) > 5000.0) {
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipGetLastError());
        break;
      }
    }
    if (ordered) {
      auto td = Clock::now();
      CHK(wait_done(sc, seq));
      if (c->timing) c->host_add(HT_WAIT_DONE, ms_since(td));
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  }
  for (uint32_t s = 0; s < nsub; ++s)
    if (hdr[s].token != token) return fail(PM_EHIP, "step results not published (sub-query " + std::to_string(s) + ")");
  if (ordered && c->rows_check)   // assertion: the completed step's bytes are the ones its headers describe
    for (uint32_t s = 0; s < nsub; ++s)
      if (row_hash(s) != hdr[s].csum)
        return fail(PM_EHIP, "step result row " + std::to_string(s) + " does not match its header after completion");
  return 0;
}

static void post_results(Engine* g, PmOutHdr* hdr, uint64_t* rows, uint32_t nsub, uint32_t base,
                         uint32_t token);
// Wait for a step's results (tokens in pinned memory) and update the host
// mirrors.
static int wait_and_post(Engine* g, const PmStep& S, uint32_t nsub, Clock::time_point) {
  pm_ctx* c = g->ctx;
  const uint64_t E = g->E;
  auto t_wait = Clock::now();
  CHK(wait_step(c, S.hdr_h, nsub, S.token, (const char*)S.rows_h, E * 8, (size_t)S.pf_w0 * 8,
                (size_t)(S.pf_w1 - S.pf_w0) * 8, g->step_seq));
  c->host_add(HT_STEP_WAIT, ms_since(t_wait));

  if (c->verify_rows) {   // diagnostics: what the host saw at token time vs after the stream drains
    std::vector<uint64_t> seen((const uint64_t*)S.rows_h, (const uint64_t*)S.rows_h + (uint64_t)nsub * E);
    std::vector<PmOutHdr> hseen(S.hdr_h, S.hdr_h + nsub);
    HIPCHK(hipStreamSynchronize(c->stream));
    for (uint32_t s = 0; s < nsub; ++s) {
      const bool rd = memcmp(seen.data() + (uint64_t)s * E, (const uint64_t*)S.rows_h + (uint64_t)s * E, E * 8) != 0;
      const bool hd = memcmp(&hseen[s], &S.hdr_h[s], sizeof(PmOutHdr)) != 0;
      if (rd || hd)
        fprintf(stderr, "[pm] verify: token %u sub %u status %u: %s%s changed after the token was seen\n", S.token, s,
                S.hdr_h[s].status, rd ? "row " : "", hd ? "header " : "");
    }
  }
  auto t_post = Clock::now();
  post_results(g, S.hdr_h, S.rows_h, nsub, 0, S.token);
  c->host_add(HT_STEP_POST, ms_since(t_post));
  return 0;
}

// The host side of a published step for one engine whose sub-queries are
// [base, base + nsub) of the step (base > 0 when several clients shared the
// step, pm_search_loop_batched): result pointers, FinishedQueryNum and
// localCache mirrors (pir.go:469-470), in-step cache hits copied from the
// earlier response (their reference is a step-wide sub-query index).
static void post_results(Engine* g, PmOutHdr* hdr, uint64_t* rows, uint32_t nsub, uint32_t base,
                         uint32_t token) {
  pm_ctx* c = g->ctx;
  const uint64_t E = g->E;
  g->hdr = hdr + base;
  g->rows = rows + (uint64_t)base * E;
  PmStep S{};
  S.token = token;
  // host mirrors: FinishedQueryNum and the localCache index (pir.go:469-470);
  // in-step cache hits copy the earlier response
  if (c->log_steps) {   // diagnostics: every sub-query of the step
    for (uint32_t s = 0; s < nsub; ++s)
      fprintf(stderr, "[pm] step %p tok %u s %u part %u kind %u idx %lu -> st %u ref %u row0 %016lx\n", (void*)g,
              S.token, s, g->subs[s].part, g->subs[s].kind, (unsigned long)g->subs[s].idx, g->hdr[s].status,
              g->hdr[s].ref, (unsigned long)g->rows[(uint64_t)s * E]);
  }
  if (c->debug_cache) {   // diagnostics: cached answers against the rows the host got for their slots
    for (uint32_t s = 0; s < nsub; ++s) {
      const PmOutHdr& h = g->hdr[s];
      PartHost& ph = g->parts[g->subs[s].part];
      const uint64_t* row = g->rows + (uint64_t)s * E;
      if (h.status == ST_OK) ph.shadow[h.ref].assign(row, row + E);
      if (h.status == ST_CACHED) {
        auto it = ph.shadow.find(h.ref);
        if (it == ph.shadow.end() || memcmp(it->second.data(), row, E * 8) != 0) {
          (void)hipStreamSynchronize(c->stream);   // diagnostics only
          std::vector<uint64_t> dev(E);
          (void)hipMemcpy(dev.data(), ph.d.arena + (uint64_t)h.ref * E, E * 8, hipMemcpyDeviceToHost);
          const bool dev_ok = it != ph.shadow.end() && memcmp(it->second.data(), dev.data(), E * 8) == 0;
          fprintf(stderr, "[pm] cache: token %u sub %u part %u idx %lu slot %u: row differs from the slot's answer%s; "
                  "device arena now %s the slot's answer; row[0] %016lx shadow[0] %016lx arena[0] %016lx\n",
                  S.token, s, g->subs[s].part, (unsigned long)g->subs[s].idx, h.ref,
                  it == ph.shadow.end() ? " (no answer recorded)" : "", dev_ok ? "equals" : "differs from",
                  (unsigned long)row[0], (unsigned long)(it == ph.shadow.end() ? 0 : it->second[0]), (unsigned long)dev[0]);
        }
      }
    }
  }
  for (uint32_t s = 0; s < nsub; ++s) {
    const PmOutHdr& h = g->hdr[s];
    if (h.status == ST_OK) {
      PartHost& ph = g->parts[g->subs[s].part];
      ph.fqn++;
      ph.cache.put(g->subs[s].idx, h.ref);
    } else if (h.status == ST_DUP) {
      const uint32_t r = h.ref - base;
      memcpy(g->rows + (uint64_t)s * E, g->rows + (uint64_t)r * E, E * 8);
      g->hdr[s].dist = g->hdr[r].dist;
    }
  }
#ifdef PM_STAMPS
  {   // partition 0's phase deltas in shader clocks, accumulated; printed at exit
    std::vector<uint64_t> t(64);
    (void)hipMemcpy(t.data(), g->buf.stamps.p, 64 * 8, hipMemcpyDeviceToHost);
    g->stamp_sum.resize(64, 0.0);
    for (int i = 1; i < 64; ++i)
    {   // each kernel's stamps relative to its own first one
      const uint64_t base = i >= 48 ? t[48] : i >= 41 ? t[41] : t[0];
      if (t[i] && base && i != 41 && i != 48) g->stamp_sum[i] += (double)(t[i] - base);
    }
    g->stamp_n++;
  }
#endif
}

static int engine_step(Engine* g, const float* q_dev, uint32_t dim) {
  auto t_begin = Clock::now();
  pm_ctx* c = g->ctx;
  hipStream_t st = c->stream;
  const uint32_t nsub = (uint32_t)g->subs.size();
  if (nsub == 0) return 0;
  const uint64_t E = g->E;
  const uint32_t words = (g->maxPH + 63) / 64, cblk = pmk::step_match_blocks(g->maxPH);
  StepBufs& B = g->buf;
  CHK(B.reserve(nsub, (uint32_t)g->P, words, cblk, E));
  const size_t dsub = nsub * sizeof(PmSub);
  CHK(B.desc_h.reserve(dsub + (g->P + 1) * 4));
  CHK(B.out_h.reserve(step_out_bytes(nsub, E)));
  char* dh = B.desc_h.as<char>();
  memcpy(dh, g->subs.data(), dsub);
  memcpy(dh + dsub, g->sb.data(), (g->P + 1) * 4);
  PmStep S{};
  S.parts = g->parts_d.as<PmPart>();
  S.subs_h = (const PmSub*)dh;
  S.sb_h = (const uint32_t*)(dh + dsub);
  B.fill(S, words, cblk);
  if (words <= g->gran_words) {   // k_step granules (sized at creation for maxPH)
    uint64_t* gb = g->gran.as<uint64_t>();
    S.recg = gb;
    S.specg = gb + kArgSubs * 8;
    S.bitsg = gb + kArgSubs * (8 + 64);
    S.resg = gb + kArgSubs * (8 + 64 + 2 * (uint64_t)g->gran_words);
    S.err_h = g->err_h.as<uint32_t>();
  }
  S.done = g->done.as<uint32_t>();
#ifdef PM_STAMPS
  CHK(B.stamps.reserve(g->P * 64 * 8));
  HIPCHK(hipMemsetAsync(B.stamps.p, 0, g->P * 64 * 8, st));
  S.stamps = B.stamps.as<uint64_t>();
#endif
  S.db = g->db->as<uint64_t>();
  S.q = q_dev;
  step_out(S, B.out_h.p, nsub);
  S.E = (uint32_t)E; S.dim = q_dev ? dim : 0; S.nsub = nsub; S.np = (uint32_t)g->P;
  S.args_valid = (nsub <= kArgSubs && g->P <= kArgParts) ? 1u : 0u;
  S.token = next_token(g->step_token);
  step_read_window(S, g->pf_off, g->pf_len, E);
  S.rows_partial = host_rows_partial(c, g->rows_partial);
  if (S.args_valid) {
    memcpy(S.subs_a, g->subs.data(), dsub);
    memcpy(S.sb_a, g->sb.data(), (g->P + 1) * 4);
  }
  uint32_t nreal = 0;
  for (auto& x : g->subs) nreal += x.kind == SUB_REAL;
  uint32_t max_per_part = 0;
  S.np_live = 0;
  for (uint64_t p = 0; p < g->P; ++p) {
    const uint32_t n = g->sb[p + 1] - g->sb[p];
    max_per_part = std::max(max_per_part, n);
    S.np_live += n > 0;
  }
  double ans_bytes = 0;
  for (auto& x : g->subs)
    if (x.kind == SUB_REAL || x.kind == SUB_DUMMY) ans_bytes += answer_bytes(g->parts[x.part].d, E);
  // One launch (k_step) when the step fits it, else the three kernels.
  // Timing level 2: the kernels carry their events in their own dispatch packets.
  if (!c->no_fuse && !c->debug_sync && pmk::step_fused_ok(S, g->maxPH, max_per_part)) {
    S.cblk = 1;   // one match workgroup per sub-query
    S.no_guess = c->no_guess ? 1u : 0u;
    // gather helpers where the launch still fits the 240 co-resident
    // workgroups (one 1,024-thread workgroup per CU): configs[2]'s 32
    // sub-queries over 16 partitions take PM_STEP_HELP (default 3) each; 0 disables
    static const int help_env = [] { const char* e = getenv("PM_STEP_HELP"); return e ? atoi(e) : 3; }();
    S.nhelp = 0;
    if (help_env > 0 && (E & ~3ull) <= kHelpWords && 2 * nsub + g->P < 240)
      S.nhelp = std::min<uint32_t>(std::min<uint32_t>(kStepHelpMax, (uint32_t)help_env),
                                   (uint32_t)((240 - 2 * nsub - g->P) / nsub));
    if (S.nhelp && !g->helpg.p) {   // the helpers' hand-off granules, on first use (token 0 never marks a step)
      const size_t nh = (size_t)kArgSubs * kStepHelpMax * kHelpGran * 8;
      CHK(g->helpg.reserve(nh));
      HIPCHK(hipMemsetAsync(g->helpg.p, 0, nh, st));
    }
    S.helpg = g->helpg.as<uint64_t>();
#ifdef PM_STEP_STAMPS
    const uint32_t grid = 2 * nsub + (uint32_t)g->P + S.nhelp * nsub;
    CHK(B.stamps.reserve((uint64_t)grid * 8 * 8));
    HIPCHK(hipMemsetAsync(B.stamps.p, 0, (uint64_t)grid * 8 * 8, st));
    S.stamps = B.stamps.as<uint64_t>();
#endif
    c->timed_ext("step", ans_bytes, [&](pmk::PmEvents ev) { pmk::step_fused(st, S, ev); }, 2);
    g->step_seq = c->record_done(st);
    HIPCHK(hipGetLastError());
    c->host_add(HT_STEP_LAUNCH, ms_since(t_begin));
    CHK(wait_and_post(g, S, nsub, t_begin));
    if (*(volatile uint32_t*)S.err_h) {
      *(volatile uint32_t*)S.err_h = 0;
      return fail(PM_EHIP, "k_step: a hand-off wait timed out (results of this step are invalid)");
    }
#ifdef PM_STEP_STAMPS
    if (const char* fn = getenv("PM_STAMP_FILE")) {   // append {grid, nsub, cblk, np} + grid x 8 stamps
      const uint32_t h[4] = {grid, nsub, cblk, (uint32_t)g->P};
      CHK(dump_stamps(st, fn, h, sizeof h, B.stamps, (uint64_t)grid * 8));
    }
#endif
    return 0;
  }
  const pmk::StepOpts opts = pmk::step_opts();
  int path = 0;
  c->timed_ext("hint_match", (double)nreal * g->maxPH, [&](pmk::PmEvents ev) { path = pmk::step_match(st, S, opts, g->ph8, g->maxPH, max_per_part, ev); }, 2);
  c->count_match_path(path);
  const bool lds = pmk::step_resolve_lds_ok(g->maxPH, max_per_part);
  c->timed_ext("resolve", 0, [&](pmk::PmEvents ev) { pmk::step_resolve(st, S, lds, ev); }, 2);
  if (c->debug_sync) {   // validate every resolution record before k_answer consumes it
    std::vector<PmRes> rr(nsub);
    HIPCHK(hipMemcpy(rr.data(), S.res, nsub * sizeof(PmRes), hipMemcpyDeviceToHost));
    for (uint32_t s = 0; s < nsub; ++s) {
      const PmPart& d = g->parts[g->subs[s].part].d;
      const PmRes& r = rr[s];
      const bool bad = (r.status == ST_OK && (r.hit >= d.PH || r.slot >= d.MaxQ || r.chunk >= d.SS || r.ing >= d.Qpc)) ||
                       (r.status == ST_CACHED && r.slot >= d.MaxQ) || (r.status == ST_DUP && r.slot >= nsub) ||
                       (r.status > ST_SKIP) || (r.status > ST_ERANGE && r.status < ST_DUMMY);
      fprintf(stderr, "[pm] res s=%u part=%u kind=%u idx=%lu -> st=%u hit=%u chunk=%u ing=%u tag=%u pp=%u slot=%u flags=%u%s\n",
              s, g->subs[s].part, g->subs[s].kind, (unsigned long)g->subs[s].idx, r.status, r.hit, r.chunk, r.ing,
              r.tag, r.pp, r.slot, r.flags, bad ? "  <-- BAD" : "");
    }
  }
  S.nsplit = c->no_split ? 1 : pmk::step_gather_split(g->maxSS, nsub);
  if (S.nsplit > 1) {
    CHK(B.part_x.reserve((uint64_t)nsub * S.nsplit * (E & ~3ull) * 8));
    S.part_x = B.part_x.as<uint64_t>();
    c->timed_ext("gather", ans_bytes, [&](pmk::PmEvents ev) { pmk::step_gather(st, S, ev); }, 2);
  }
  c->timed_ext("answer", S.nsplit > 1 ? 0 : ans_bytes, [&](pmk::PmEvents ev) { pmk::step_answer(st, S, g->maxSS, ev); }, 2);
  g->step_seq = c->record_done(st);
  HIPCHK(hipGetLastError());
  c->host_add(HT_STEP_LAUNCH, ms_since(t_begin));
  return wait_and_post(g, S, nsub, t_begin);
}

// Append one sub-query of partition p to the step being built.
static void add_sub(Engine* g, uint32_t p, bool real, uint64_t local, uint64_t gid) {
  PartHost& ph = g->parts[p];
  if (!ph.owned) return;   // another shard answers this partition
  PmSub s{p, SUB_NONE, 0};
  if (!real) {
    s.kind = SUB_DUMMY; s.idx = ph.dummy_ctr++;
  } else {
    s.kind = SUB_REAL; s.idx = local;
    if (const uint32_t* slot = ph.cache.find(local)) { s.kind = SUB_HOSTCACHE; s.idx = *slot; }
  }
  g->subs.push_back(s);
  g->sub_gid.push_back(gid);
}
static void begin_step(Engine* g) {
  g->subs.clear(); g->sub_gid.clear();
  g->sb.assign(g->P + 1, 0);
}
static void close_partition(Engine* g, uint32_t p) {   // sub_begin[p+1] = current size
  for (uint64_t i = p + 1; i <= g->P; ++i) g->sb[i] = (uint32_t)g->subs.size();
}

// ---------------------------------------------------------------------------
// PianoPIR C ABI
// ---------------------------------------------------------------------------
static void print_stamps(const Engine& e) {
#ifdef PM_STAMPS
  if (!e.stamp_n) return;
  fprintf(stderr, "[pm-stamps] mean shader clocks since kernel start over %lu steps (1-40 k_resolve part 0, 42-47 k_match, 49-63 k_answer):", (unsigned long)e.stamp_n);
  for (size_t i = 1; i < e.stamp_sum.size(); ++i)
    if (e.stamp_sum[i] > 0) fprintf(stderr, " %zu:%.0f", i, e.stamp_sum[i] / e.stamp_n);
  fprintf(stderr, "\n");
#else
  (void)e;
#endif
}
struct pm_pir { Engine e; ~pm_pir() { print_stamps(e); } };
struct pm_batchpir { Engine e; ~pm_batchpir() { print_stamps(e); } };

extern "C" int pm_pir_create(pm_ctx* ctx, uint64_t DBSize, uint64_t DBEntryByteNum, const uint64_t* rawDB,
                             uint64_t F, uint64_t seed, pm_pir** out) {
  if (!out) return fail(PM_EINVAL, "out is NULL");
  pm_pir* h = new pm_pir();
  int r = engine_create(ctx, &h->e, DBSize, DBEntryByteNum, 0, rawDB, F, seed, false);
  if (r) { delete h; return r; }
  *out = h;
  return 0;
}
extern "C" void pm_pir_destroy(pm_pir* h) { delete h; }
extern "C" int pm_pir_preprocessing(pm_pir* h) { return engine_prep(&h->e, 0, 1); }
// Initialization only (pir.go:520-523); skipPrep stays set for later preprocessing.
extern "C" int pm_pir_dummy_preprocessing(pm_pir* h) {
  h->e.skipPrep = true;
  return engine_prep(&h->e, 0, 1);
}

static int status_to_api(uint32_t st) {
  switch (st) {
    case ST_OK: case ST_DUP: case ST_CACHED: case ST_DUMMY: return PM_Q_OK;
    case ST_EBUDGET: return PM_Q_EBUDGET;
    case ST_ECHUNK: return PM_Q_ECHUNK;
    case ST_ENOHIT: return PM_Q_ENOHIT;
    default: return PM_Q_ERANGE;
  }
}

// PianoPIR.Query (pir.go:525-533) -> Client.Query (:354-471)
extern "C" int pm_pir_query(pm_pir* h, uint64_t idx, int real, uint64_t* out, int* status) {
  Engine* g = &h->e;
  PartHost& ph = g->parts[0];
  if (ph.fqn == ph.maxq64) CHK(engine_prep(g, 0, 1));
  memset(out, 0, g->E * 8);
  if (real && idx >= ph.d.N) { if (status) *status = PM_Q_ERANGE; return 0; }
  begin_step(g);
  add_sub(g, 0, real != 0, idx, idx);
  close_partition(g, 0);
  CHK(engine_step(g, nullptr, 0));
  const uint32_t st = g->hdr[0].status;
  if (st == ST_OK || st == ST_DUP || st == ST_CACHED) memcpy(out, g->rows, g->E * 8);
  if (status) *status = status_to_api(st);
  return 0;
}
extern "C" int pm_pir_config_get(pm_pir* h, pm_pir_config* c) {
  const Engine& g = h->e; const PartHost& p = g.parts[0];
  c->DBEntryByteNum = g.Ebytes; c->DBEntrySize = g.E; c->DBSize = p.d.N; c->ChunkSize = p.d.CS;
  c->SetSize = p.d.SS; c->ThreadNum = 8; c->FailureProbLog2 = g.F; c->MaxQueryNum = p.maxq64;
  c->PrimaryHintNum = p.d.PH; c->MaxQueryPerChunk = p.d.Qpc; c->FinishedQueryNum = p.fqn;
  return 0;
}
extern "C" double pm_pir_local_storage(pm_pir* h) { return part_storage(h->e.parts[0], h->e.Ebytes); }
extern "C" double pm_pir_comm_per_query(pm_pir* h) { return part_comm(h->e.parts[0], h->e.E); }

extern "C" int pm_pir_server_answer(pm_pir* h, const uint32_t* offsets, uint64_t nq, uint64_t* out) {
  Engine* g = &h->e;
  pm_ctx* c = g->ctx;
  const PmPart& d = g->parts[0].d;
  if (nq == 0) return 0;
  CHK(g->qoffs.reserve(nq * d.SS * 4));
  CHK(g->ans_srv.reserve(nq * g->E * 8));
  CHK(upload_parts(g));
  HIPCHK(hipMemcpyAsync(g->qoffs.p, offsets, nq * d.SS * 4, hipMemcpyHostToDevice, c->stream));
  c->timed("answer", (double)nq * answer_bytes(d, g->E), [&] {
    pmk::server_answer(c->stream, g->parts_d.as<PmPart>(), g->qoffs.as<uint32_t>(), (uint32_t)nq, d.SS,
                       g->db->as<uint64_t>(), (uint32_t)g->E, g->ans_srv.as<uint64_t>());
  });
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, g->ans_srv.p, nq * g->E * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

static int engine_export(Engine* g, uint64_t p, uint32_t* rk, uint64_t* pt, uint64_t* par, uint64_t* ppo,
                         uint64_t* bt, uint64_t* bpar, uint64_t* ri, uint64_t* rv, uint64_t* hist) {
  if (p >= g->P) return fail(PM_EINVAL, "partition out of range");
  const PmPart& d = g->parts[p].d;
  const uint64_t E = g->E, nb = (uint64_t)d.SS * d.Qpc;
  HIPCHK(hipStreamSynchronize(g->ctx->stream));
  if (rk) memcpy(rk, d.rk, 44 * 4);
  auto widen = [&](uint64_t* dst, const uint32_t* src, uint64_t n) -> int {
    if (!dst) return 0;
    std::vector<uint32_t> t(n);
    HIPCHK(hipMemcpy(t.data(), src, n * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n; ++i) dst[i] = t[i];
    return 0;
  };
  CHK(widen(pt, d.tag, d.PH));
  CHK(widen(ppo, d.pp, d.PH));
  CHK(widen(bt, d.tag + d.PH, nb));
  CHK(widen(ri, d.ridx, nb));
  CHK(widen(hist, d.hist, d.SS));
  if (par) HIPCHK(hipMemcpy(par, d.parity, (uint64_t)d.PH * E * 8, hipMemcpyDeviceToHost));
  if (bpar) HIPCHK(hipMemcpy(bpar, d.parity + (uint64_t)d.PH * E, nb * E * 8, hipMemcpyDeviceToHost));
  if (rv) HIPCHK(hipMemcpy(rv, d.rval, nb * E * 8, hipMemcpyDeviceToHost));
  return 0;
}
extern "C" int pm_pir_export(pm_pir* h, uint32_t* rk, uint64_t* pt, uint64_t* par, uint64_t* pp,
                             uint64_t* bt, uint64_t* bpar, uint64_t* ri, uint64_t* rv, uint64_t* hist) {
  return engine_export(&h->e, 0, rk, pt, par, pp, bt, bpar, ri, rv, hist);
}

// ---------------------------------------------------------------------------
// SimpleBatchPianoPIR C ABI (batch-pir.go)
// ---------------------------------------------------------------------------
static void record_stats(Engine* g, double t) {   // RecordStats batch-pir.go:110-117
  g->prepTime = t;
  double s = 0; for (auto& p : g->parts) s += part_storage(p, g->Ebytes);
  g->storage = (double)(uint64_t)s;
  double on = 0; for (auto& p : g->parts) on += part_comm(p, g->E) * 2.0;
  g->commOn = (double)(uint64_t)on;
  g->Support = g->parts[0].maxq64 / 2;
  double dbBytes = (double)g->N * (double)g->Ebytes;
  g->commOff = (double)(uint64_t)(dbBytes / (double)g->Support);
}
extern "C" int pm_batchpir_create(pm_ctx* ctx, uint64_t DBSize, uint64_t DBEntryByteNum, uint64_t BatchSize,
                                  const uint64_t* rawDB, uint64_t F, uint64_t seed, pm_batchpir** out) {
  return pm_batchpir_create_shard(ctx, DBSize, DBEntryByteNum, BatchSize, rawDB, F, seed, 0, 1, out);
}
extern "C" int pm_batchpir_create_shard(pm_ctx* ctx, uint64_t DBSize, uint64_t DBEntryByteNum,
                                        uint64_t BatchSize, const uint64_t* rawDB, uint64_t F, uint64_t seed,
                                        uint32_t shard, uint32_t nshards, pm_batchpir** out) {
  if (!out) return fail(PM_EINVAL, "out is NULL");
  pm_batchpir* h = new pm_batchpir();
  int r = engine_create(ctx, &h->e, DBSize, DBEntryByteNum, BatchSize, rawDB, F, seed, true, shard, nshards);
  if (r) { delete h; return r; }
  *out = h;
  return 0;
}
extern "C" int pm_batchpir_create_synth(pm_ctx* ctx, uint64_t DBSize, uint64_t DBEntryByteNum,
                                        uint64_t BatchSize, uint64_t FailureProbLog2, uint64_t seed,
                                        uint64_t db_seed, uint32_t shard, uint32_t nshards, pm_batchpir** out) {
  if (!out) return fail(PM_EINVAL, "out is NULL");
  pm_batchpir* h = new pm_batchpir();
  const DbGen gen{0, db_seed, 0, 0};
  int r = engine_create(ctx, &h->e, DBSize, DBEntryByteNum, BatchSize, nullptr, FailureProbLog2, seed, true, shard,
                        nshards, nullptr, &gen);
  if (r) { delete h; return r; }
  *out = h;
  return 0;
}
extern "C" int pm_batchpir_create_client(pm_ctx* ctx, pm_batchpir* server, uint64_t seed, pm_batchpir** out) {
  if (!out || !server) return fail(PM_EINVAL, "NULL argument");
  const Engine& s = server->e;
  pm_batchpir* h = new pm_batchpir();
  int r = engine_create(ctx, &h->e, s.N, s.Ebytes, s.B, nullptr, s.F, seed, true, s.shard, s.nshards, &s);
  if (r) { delete h; return r; }
  h->e.pf_off = s.pf_off; h->e.pf_len = s.pf_len;
  *out = h;
  return 0;
}
extern "C" void pm_batchpir_destroy(pm_batchpir* h) { delete h; }
static int batch_prep(Engine* g) {   // Preprocessing (batch-pir.go:119-155)
  g->FBN = 0; g->QMIP = 0;
  auto t0 = std::chrono::steady_clock::now();
  CHK(engine_prep(g, 0, g->P));
  double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  g->prepCount++;
  record_stats(g, t);
  return 0;
}
extern "C" int pm_batchpir_preprocessing(pm_batchpir* h) { return batch_prep(&h->e); }
extern "C" int pm_batchpir_dummy_preprocessing(pm_batchpir* h) {   // batch-pir.go:157-166
  h->e.skipPrep = true;
  CHK(engine_prep(&h->e, 0, h->e.P));
  record_stats(&h->e, 0);
  return 0;
}

// Query (batch-pir.go:170-248).  Partitions whose FinishedQueryNum cannot reach
// MaxQueryNum inside this batch run as fused steps (at most
// step_max_sub_per_part() sub-queries per partition per step); the rest replay
// the reference's per-sub-query re-preprocessing check (pir.go:527-530) one
// sub-query at a time.  q_dev / dist_out: optional L2 of every answer to q.
// Query (batch-pir.go:170-248).  Responses go to out[n][E], or, when rows_out
// is given, rows_out[i] points at response i (pinned result rows of the step,
// the collected rows of a multi-step query, or a zero row); valid until the
// next query on this engine.
static int batch_query_impl(Engine* g, const uint64_t* idx, uint64_t n, uint64_t* out, const float* q_dev,
                            uint32_t dim, float* dist_out, const uint64_t** rows_out, uint8_t* ok);
static int batch_query(Engine* g, const uint64_t* idx, uint64_t n, uint64_t* out, const float* q_dev,
                       uint32_t dim, float* dist_out, const uint64_t** rows_out = nullptr,
                       uint8_t* ok = nullptr) {
  auto t = Clock::now();
  int r = batch_query_impl(g, idx, n, out, q_dev, dim, dist_out, rows_out, ok);
  g->ctx->host_add(HT_BATCH_QUERY, ms_since(t));
  return r;
}
static inline bool status_ok(uint32_t st) { return st == ST_OK || st == ST_CACHED || st == ST_DUP; }

// SimpleBatchPianoPIR.Query (batch-pir.go:170-248) in three parts, so that a
// driver serving several clients can put many clients' steps in one launch
// (pm_search_loop_batched):
//   bq_prepare   bucketing (:176-200): ids per partition, dummy padding,
//                overflow drop; when every partition is clear of its query
//                budget (the usual case), the one step's sub-queries
//                (*fast = true);
//   bq_emit_fast after that step is published: each id's response (the last
//                one made for it, :187,213), distance and success flag;
//   bq_tail      FinishedBatchNum / QueriesMadeInPartition and the
//                re-preprocessing trigger (:238-247).
static int bq_prepare(Engine* g, const uint64_t* idx, uint64_t n, bool* fast) {
  const uint64_t E = g->E, P = g->P;
  CHK(ensure_host_cache(g));
  if (g->zero_row.size() != E) g->zero_row.assign(E, 0);
  for (uint64_t i = 0; i < n; ++i)
    if (idx[i] >= g->N) return fail(PM_EINVAL, "id " + std::to_string(idx[i]) + " >= DBSize");
  const uint64_t qn = n / P;
  g->qn = qn;
  g->pq.resize(P);
  for (auto& v : g->pq) v.clear();
  for (uint64_t i = 0; i < n; ++i) g->pq[g->part_of(idx[i])].push_back(idx[i]);
  for (auto& v : g->pq) while (v.size() < qn) v.push_back(kDefaultValue);
  g->resp_map.clear();
  g->resp_rows.resize(std::max<size_t>(g->resp_rows.size(), n * E));
  g->resp_dist.resize(std::max<size_t>(g->resp_dist.size(), n));
  g->resp_ok.resize(std::max<size_t>(g->resp_ok.size(), n));
  g->slow.assign(P, 0);
  bool any_slow = false;
  for (uint64_t p = 0; p < P; ++p) {
    uint64_t nreal = 0;
    for (uint64_t j = 0; j < qn; ++j) nreal += g->pq[p][j] != kDefaultValue;
    const PartHost& ph = g->parts[p];
    g->slow[p] = qn && ph.fqn + nreal >= ph.maxq64;
    any_slow |= g->slow[p] != 0;
  }
  *fast = !any_slow && qn <= pmk::step_max_sub_per_part() && qn > 0;
  if (*fast) {
    // the localCache slots every real sub-query looks up (add_sub), requested
    // together: the session's state is cold when the serving loop reaches it
    for (uint64_t p = 0; p < P; ++p)
      if (g->parts[p].owned)
        for (uint64_t j = 0; j < qn; ++j)
          if (g->pq[p][j] != kDefaultValue) g->parts[p].cache.prefetch(g->pq[p][j] - p * g->PS);
    begin_step(g);
    for (uint64_t p = 0; p < P; ++p) {
      for (uint64_t j = 0; j < qn; ++j) {
        const uint64_t id = g->pq[p][j];
        add_sub(g, (uint32_t)p, id != kDefaultValue, id - p * g->PS, id);
      }
      close_partition(g, (uint32_t)p);
    }
  }
  return 0;
}
static void bq_emit_fast(Engine* g, const uint64_t* idx, uint64_t n, uint64_t* out, float* dist_out,
                         const uint64_t** rows_out, uint8_t* ok) {
  const uint64_t E = g->E;
  for (size_t s = 0; s < g->subs.size(); ++s) {
    const uint32_t k = g->subs[s].kind;
    if (k == SUB_REAL || k == SUB_HOSTCACHE) g->resp_map.put(g->sub_gid[s], (uint32_t)s);   // last wins
  }
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t* sp = g->resp_map.find(idx[i]);
    const uint64_t* row = sp ? g->rows + (uint64_t)*sp * E : g->zero_row.data();
    if (rows_out) rows_out[i] = row;
    else memcpy(out + i * E, row, E * 8);
    if (dist_out) dist_out[i] = sp ? g->hdr[*sp].dist : 0.0f;
    if (ok) ok[i] = sp && status_ok(g->hdr[*sp].status);
  }
}
static int bq_tail(Engine* g, uint64_t n) {
  if (g->QMIP >= g->parts[0].maxq64 - 2) {
    CHK(batch_prep(g));
  } else {
    g->FBN += n / g->B;
    g->QMIP += g->qn;
  }
  return 0;
}
static int batch_query_impl(Engine* g, const uint64_t* idx, uint64_t n, uint64_t* out, const float* q_dev,
                            uint32_t dim, float* dist_out, const uint64_t** rows_out, uint8_t* ok) {
  const uint64_t E = g->E, P = g->P;
  bool fast = false;
  CHK(bq_prepare(g, idx, n, &fast));
  const uint64_t qn = g->qn;
  if (fast) {   // common case: one step; ids map straight onto the pinned result rows
    CHK(engine_step(g, q_dev, dim));
    bq_emit_fast(g, idx, n, out, dist_out, rows_out, ok);
    return bq_tail(g, n);
  }
  size_t nresp = 0;
  auto collect = [&]() {
    for (size_t s = 0; s < g->subs.size(); ++s) {
      const uint32_t k = g->subs[s].kind;
      if (k != SUB_REAL && k != SUB_HOSTCACHE) continue;
      if (g->resp_map.emplace(g->sub_gid[s], (uint32_t)nresp)) ++nresp;
      const uint32_t slot = *g->resp_map.find(g->sub_gid[s]);
      memcpy(&g->resp_rows[(size_t)slot * E], g->rows + (uint64_t)s * E, E * 8);
      g->resp_dist[slot] = g->hdr[s].dist;
      g->resp_ok[slot] = status_ok(g->hdr[s].status);
    }
  };
  const uint64_t kStep = pmk::step_max_sub_per_part();
  for (uint64_t j0 = 0; j0 < qn; j0 += kStep) {
    const uint64_t j1 = std::min(qn, j0 + kStep);
    begin_step(g);
    for (uint64_t p = 0; p < P; ++p) {
      if (!g->slow[p])
        for (uint64_t j = j0; j < j1; ++j) {
          const uint64_t id = g->pq[p][j];
          add_sub(g, (uint32_t)p, id != kDefaultValue, id - p * g->PS, id);
        }
      close_partition(g, (uint32_t)p);
    }
    if (!g->subs.empty()) { CHK(engine_step(g, q_dev, dim)); collect(); }
  }
  for (uint64_t p = 0; p < P; ++p) {
    if (!g->slow[p]) continue;
    for (uint64_t j = 0; j < qn; ++j) {
      PartHost& ph = g->parts[p];
      if (ph.fqn == ph.maxq64) CHK(engine_prep(g, p, p + 1));
      begin_step(g);
      const uint64_t id = g->pq[p][j];
      add_sub(g, (uint32_t)p, id != kDefaultValue, id - p * g->PS, id);
      close_partition(g, (uint32_t)p);
      CHK(engine_step(g, q_dev, dim));
      collect();
    }
  }
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t* sp = g->resp_map.find(idx[i]);
    const uint64_t* row = sp ? &g->resp_rows[(size_t)*sp * E] : g->zero_row.data();
    if (rows_out) rows_out[i] = row;
    else memcpy(out + i * E, row, E * 8);
    if (dist_out) dist_out[i] = sp ? g->resp_dist[*sp] : 0.0f;
    if (ok) ok[i] = sp && g->resp_ok[*sp];
  }
  return bq_tail(g, n);
}
// the slow path of pm_batchpir_query_dev: batch_query_impl's response rows (host) and flags
static int batch_query_impl_rows(Engine* g, const uint64_t* idx, uint64_t n, const uint64_t** rows_out, uint8_t* ok) {
  return batch_query_impl(g, idx, n, nullptr, nullptr, 0, nullptr, rows_out, ok);
}
extern "C" int pm_batchpir_query(pm_batchpir* h, const uint64_t* ids, uint64_t n, uint64_t* out) {
  return batch_query(&h->e, ids, n, out, nullptr, 0, nullptr);
}
extern "C" int pm_batchpir_query_ok(pm_batchpir* h, const uint64_t* ids, uint64_t n, uint64_t* out,
                                    uint8_t* ok) {
  return batch_query(&h->e, ids, n, out, nullptr, 0, nullptr, nullptr, ok);
}
// Query with the responses left in device memory for an in-place collective
// (the sharded combine): a successful sub-query's entry is the
// row k_answer stored in its partition's localCache arena (slot = the
// resolution's, followed through in-step duplicates), so the responses are
// copied HBM to HBM by one k_gather_rows launch; only the row pointers come
// from the host.  A query that needed several steps (a partition at its budget
// mid-batch, pir.go:527-530) has its rows in host memory and uploads them.
static int query_dev_impl(Engine* g, const uint64_t* ids, uint64_t n, uint64_t* dev_out, hipStream_t cs);
extern "C" int pm_batchpir_query_dev(pm_batchpir* h, const uint64_t* ids, uint64_t n, uint64_t* dev_out,
                                     void* stream) {
  Engine* g = &h->e;
  if (n && (!ids || !dev_out)) return fail(PM_EINVAL, "NULL argument");
  auto t = Clock::now();
  const int r = query_dev_impl(g, ids, n, dev_out, (hipStream_t)stream);
  g->ctx->host_add(HT_BATCH_QUERY, ms_since(t));
  return r;
}
static int query_dev_impl(Engine* g, const uint64_t* ids, uint64_t n, uint64_t* dev_out, hipStream_t cs) {
  const uint64_t E = g->E;
  hipStream_t st = g->ctx->stream;
  HIPCHK(hipSetDevice(g->ctx->device));
  if (!g->dev_ev) HIPCHK(hipEventCreateWithFlags(&g->dev_ev, hipEventDisableTiming));
  // dev_out may still be read by work the consumer queued before this call
  // (its last collective, a kernel on the previous rows): the engine's writes
  // into it wait for that work (stream order, no host synchronisation)
  if (cs) {
    HIPCHK(hipEventRecord(g->dev_ev, cs));
    HIPCHK(hipStreamWaitEvent(st, g->dev_ev, 0));
  }
  bool fast = false;
  CHK(bq_prepare(g, ids, n, &fast));
  if (fast) {
    CHK(engine_step(g, nullptr, 0));
    for (size_t s = 0; s < g->subs.size(); ++s) {
      const uint32_t k = g->subs[s].kind;
      if (k == SUB_REAL || k == SUB_HOSTCACHE) g->resp_map.put(g->sub_gid[s], (uint32_t)s);   // last wins
    }
    CHK(g->src_h.reserve(std::max<uint64_t>(1, n) * 8));
    const uint64_t** src = g->src_h.as<const uint64_t*>();
    for (uint64_t i = 0; i < n; ++i) {
      src[i] = nullptr;
      const uint32_t* sp = g->resp_map.find(ids[i]);
      if (!sp) continue;
      uint32_t s = *sp;
      for (int hop = 0; g->hdr[s].status == ST_DUP && hop < 2; ++hop) s = g->hdr[s].ref;   // step-wide index
      const uint32_t stt = g->hdr[s].status;
      if (stt == ST_OK || stt == ST_CACHED)
        src[i] = g->parts[g->subs[s].part].d.arena + (uint64_t)g->hdr[s].ref * E;
    }
    pmk::gather_rows(st, src, n, (uint32_t)E, dev_out);
    HIPCHK(hipGetLastError());
  } else {   // rows collected on the host by the multi-step path (a partition at its budget mid-batch)
    std::vector<uint8_t> ok(n);
    std::vector<const uint64_t*> rp(n);
    CHK(batch_query_impl_rows(g, ids, n, rp.data(), ok.data()));   // runs the re-preprocessing trigger itself
    // staged in pinned memory: the copy is asynchronous, so the staging buffer
    // must outlive this call (it is the engine's; the next call's copy is
    // ordered after this one on the same stream)
    HIPCHK(hipStreamSynchronize(st));   // the previous call's copy out of stage_h is done
    CHK(g->stage_h.reserve(std::max<uint64_t>(1, n) * (E + 1) * 8));
    uint64_t* rows = g->stage_h.as<uint64_t>();
    for (uint64_t i = 0; i < n; ++i) {
      memcpy(&rows[i * (E + 1)], rp[i], E * 8);
      rows[i * (E + 1) + E] = ok[i];
    }
    HIPCHK(hipMemcpyAsync(dev_out, rows, n * (E + 1) * 8, hipMemcpyHostToDevice, st));
  }
  if (cs) {   // the consumer's stream waits for the rows; no host synchronisation
    HIPCHK(hipEventRecord(g->dev_ev, st));
    HIPCHK(hipStreamWaitEvent(cs, g->dev_ev, 0));
  } else {
    HIPCHK(hipStreamSynchronize(st));
  }
  return fast ? bq_tail(g, n) : 0;   // stream-ordered after the copy
}
extern "C" int pm_batchpir_stats_get(pm_batchpir* h, pm_batchpir_stats* s) {
  const Engine& g = h->e;
  s->DBEntryByteNum = g.Ebytes; s->DBEntrySize = g.E; s->DBSize = g.N; s->BatchSize = g.B;
  s->PartitionNum = g.P; s->PartitionSize = g.PS; s->ThreadNum = 1; s->FailureProbLog2 = g.F;
  s->FinishedBatchNum = g.FBN; s->QueriesMadeInPartition = g.QMIP; s->SupportBatchNum = g.Support;
  s->PrepCount = g.prepCount; s->LocalStorage = g.storage; s->PreprocessingTime = g.prepTime;
  s->CommOnline = g.commOn; s->CommOffline = g.commOff;
  return 0;
}
extern "C" int pm_batchpir_subconfig(pm_batchpir* h, uint64_t p, pm_pir_config* c) {
  const Engine& g = h->e;
  if (p >= g.P) return fail(PM_EINVAL, "partition out of range");
  const PartHost& ph = g.parts[p];
  c->DBEntryByteNum = g.Ebytes; c->DBEntrySize = g.E; c->DBSize = ph.d.N; c->ChunkSize = ph.d.CS;
  c->SetSize = ph.d.SS; c->ThreadNum = 8; c->FailureProbLog2 = g.F; c->MaxQueryNum = ph.maxq64;
  c->PrimaryHintNum = ph.d.PH; c->MaxQueryPerChunk = ph.d.Qpc; c->FinishedQueryNum = ph.fqn;
  return 0;
}
extern "C" int pm_batchpir_export(pm_batchpir* h, uint64_t p, uint32_t* rk, uint64_t* pt, uint64_t* par,
                                  uint64_t* pp, uint64_t* bt, uint64_t* bpar, uint64_t* ri, uint64_t* rv,
                                  uint64_t* hist) {
  if (p >= h->e.P || !h->e.parts[p].owned) return fail(PM_EINVAL, "partition not held by this shard");
  return engine_export(&h->e, p, rk, pt, par, pp, bt, bpar, ri, rv, hist);
}

// ---------------------------------------------------------------------------
// graphann: GraphANNFrontend over PIRGraphInfo / BasicGraphInfo
// ---------------------------------------------------------------------------
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
static int check_session(const pm_graph* g) {
  if (!g->lost.empty()) return fail(PM_EINVAL, "session state lost: " + g->lost);
  return 0;
}

// PIRGraphInfo over one shard of the graph DB (multi-GPU private search,
// SURVEY.md §8e): host vectors and graph as pm_graph_create, but only the
// partitions p % nshards == shard are uploaded and served by this handle.
extern "C" int pm_graph_create_shard(pm_ctx* ctx, uint64_t n, uint64_t dim, uint64_t m, const float* vectors,
                                     const uint32_t* graph, uint32_t shard, uint32_t nshards, uint64_t pir_seed,
                                     uint64_t search_seed, pm_graph** out) {
  if (!ctx || !out || !vectors || !graph) return fail(PM_EINVAL, "NULL argument");
  if (n == 0 || dim == 0 || m == 0) return fail(PM_EINVAL, "n, dim, m must be > 0");
  if ((dim * 4 + m * 4) % 8) return fail(PM_EINVAL, "(4*dim + 4*m) must be a multiple of 8");
  if (nshards == 0 || shard >= nshards) return fail(PM_EINVAL, "shard must be < nshards");
  HIPCHK(hipSetDevice(ctx->device));
  pm_graph* g = new pm_graph();
  g->ctx = ctx; g->n = n; g->dim = dim; g->m = m;
  g->pir_seed = pir_seed; g->rng.s = search_seed;
  g->shard = shard; g->nshards = nshards;
  g->vec_own = std::make_shared<const std::vector<float>>(vectors, vectors + n * dim);
  g->graph_own = std::make_shared<const std::vector<uint32_t>>(graph, graph + n * m);
  g->vectors = g->vec_own->data();
  g->graph = g->graph_own->data();
  if (int r = g->dq.reserve(dim * 4)) { delete g; return r; }
  *out = g;
  return 0;
}
// The same over the synthetic graph (graph_synth_elem of data_seed, the
// reference's -input synthetic mode) generated on the device: BIGANN-scale
// graph DBs that cannot be built or shipped (BASELINE.json configs[3]/[4]).
extern "C" int pm_graph_create_synth(pm_ctx* ctx, uint64_t n, uint64_t dim, uint64_t m, uint64_t data_seed,
                                     uint32_t shard, uint32_t nshards, uint64_t pir_seed, uint64_t search_seed,
                                     pm_graph** out) {
  if (!ctx || !out) return fail(PM_EINVAL, "NULL argument");
  if (n <= 1 || dim == 0 || m == 0 || m > 64 || n > 0xffffffffull)
    return fail(PM_EINVAL, "need 1 < n < 2^32, dim > 0, 0 < m <= 64");
  if ((dim + m) % 2) return fail(PM_EINVAL, "(4*dim + 4*m) must be a multiple of 8");
  if (nshards == 0 || shard >= nshards) return fail(PM_EINVAL, "shard must be < nshards");
  HIPCHK(hipSetDevice(ctx->device));
  pm_graph* g = new pm_graph();
  g->ctx = ctx; g->n = n; g->dim = dim; g->m = m;
  g->pir_seed = pir_seed; g->rng.s = search_seed;
  g->shard = shard; g->nshards = nshards;
  g->synth = true; g->data_seed = data_seed;
  if (int r = g->dq.reserve(dim * 4)) { delete g; return r; }
  *out = g;
  return 0;
}
// Host restatement of the synthetic graph's rows (tests, checks): vec[i*dim..]
// and nb[i*m..] of vertex ids[i]; either output may be NULL.
extern "C" int pm_graph_synth_rows(uint64_t n, uint64_t dim, uint64_t m, uint64_t data_seed, const uint64_t* ids,
                                   uint64_t k, float* vec, uint32_t* nb) {
  if (k && !ids) return fail(PM_EINVAL, "NULL argument");
  const uint64_t kv = sm64(data_seed + DOM_SYNTH_VEC), kg = sm64(data_seed + DOM_SYNTH_NB);
  for (uint64_t i = 0; i < k; ++i) {
    if (ids[i] >= n) return fail(PM_EINVAL, "id out of range");
    if (vec) for (uint64_t j = 0; j < dim; ++j) vec[i * dim + j] = graph_synth_vec(kv, ids[i], (uint32_t)dim, (uint32_t)j);
    if (nb) for (uint64_t j = 0; j < m; ++j) nb[i * m + j] = graph_synth_nb(kg, n, ids[i], (uint32_t)m, (uint32_t)j);
  }
  return 0;
}

extern "C" int pm_graph_create(pm_ctx* ctx, uint64_t n, uint64_t dim, uint64_t m, const float* vectors,
                               const uint32_t* graph, int nonprivate, int skip_prep, uint64_t pir_seed,
                               uint64_t search_seed, pm_graph** out) {
  if (!ctx || !out || !vectors || !graph) return fail(PM_EINVAL, "NULL argument");
  if (n == 0 || dim == 0 || m == 0) return fail(PM_EINVAL, "n, dim, m must be > 0");
  if ((dim * 4 + m * 4) % 8) return fail(PM_EINVAL, "(4*dim + 4*m) must be a multiple of 8");
  HIPCHK(hipSetDevice(ctx->device));
  pm_graph* g = new pm_graph();
  g->ctx = ctx; g->n = n; g->dim = dim; g->m = m; g->nonprivate = nonprivate; g->skipPrep = skip_prep;
  g->pir_seed = pir_seed; g->rng.s = search_seed;
  g->vec_own = std::make_shared<const std::vector<float>>(vectors, vectors + n * dim);
  g->graph_own = std::make_shared<const std::vector<uint32_t>>(graph, graph + n * m);
  g->vectors = g->vec_own->data();
  g->graph = g->graph_own->data();
  int r = g->dvec->reserve(n * dim * 4);
  if (!r) r = g->dq.reserve(dim * 4);
  if (r) { delete g; return r; }
  hipError_t e = hipMemcpy(g->dvec->p, vectors, n * dim * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) { delete g; return fail(PM_EHIP, hipGetErrorString(e)); }
  *out = g;
  return 0;
}
// A second client session over the same graph and server: shares the host
// vectors/graph, their device copy and (after pm_graph_preprocess) the server
// DB of `base`'s batch PIR, with its own context, keys, hint state, start set
// and id stream.  `base` must be preprocessed and outlive its sessions' preprocessing.
extern "C" int pm_graph_create_session(pm_ctx* ctx, pm_graph* base, uint64_t pir_seed, uint64_t search_seed,
                                       pm_graph** out) {
  if (!ctx || !base || !out) return fail(PM_EINVAL, "NULL argument");
  if (!base->nonprivate && !base->pir) return fail(PM_EINVAL, "base graph not preprocessed");
  if (base->ctx->device != ctx->device) return fail(PM_EINVAL, "a session shares its base's device");
  HIPCHK(hipSetDevice(ctx->device));
  pm_graph* g = new pm_graph();
  g->ctx = ctx; g->n = base->n; g->dim = base->dim; g->m = base->m;
  g->nonprivate = base->nonprivate; g->skipPrep = base->skipPrep;
  g->pir_seed = pir_seed; g->rng.s = search_seed;
  g->vec_own = base->vec_own; g->graph_own = base->graph_own;
  g->vectors = base->vectors; g->graph = base->graph;
  g->dvec = base->dvec;
  g->dgraph = base->dgraph;
  g->shard = base->shard; g->nshards = base->nshards;
  g->synth = base->synth; g->data_seed = base->data_seed;
  g->server = base->pir;
  if (int r = g->dq.reserve(g->dim * 4)) { delete g; return r; }
  *out = g;
  return 0;
}
extern "C" void pm_graph_destroy(pm_graph* g) { delete g; }
extern "C" pm_batchpir* pm_graph_pir(pm_graph* g) { return g->pir; }
extern "C" int pm_graph_counts(pm_graph* g, uint64_t* t, uint64_t* s) { *t = g->total; *s = g->succ; return 0; }

// PIRGraphInfo.Preprocess (private-search.go:355-412) + GetStartVertex (:508-531)
extern "C" int pm_graph_preprocess(pm_graph* g) {
  if (g->server) {   // session: a new client over the base's server DB
    delete g->pir; g->pir = nullptr;
    CHK(pm_batchpir_create_client(g->ctx, g->server, g->pir_seed, &g->pir));
    if (g->skipPrep) CHK(pm_batchpir_dummy_preprocessing(g->pir));
    else CHK(pm_batchpir_preprocessing(g->pir));
  } else if (g->synth) {   // the synthetic graph's entries generated on the device, this shard's partitions
    const uint64_t ebytes = g->dim * 4 + g->m * 4;
    delete g->pir; g->pir = nullptr;
    pm_batchpir* h = new pm_batchpir();
    const DbGen gen{1, g->data_seed, (uint32_t)g->dim, (uint32_t)g->m};
    if (int r = engine_create(g->ctx, &h->e, g->n, ebytes, g->m, nullptr, 8, g->pir_seed, true, g->shard, g->nshards,
                              nullptr, &gen)) { delete h; return r; }
    g->pir = h;
    g->pir->e.pf_off = g->dim * 4;
    g->pir->e.pf_len = g->m * 4;
    if (g->skipPrep) CHK(pm_batchpir_dummy_preprocessing(g->pir));
    else CHK(pm_batchpir_preprocessing(g->pir));
  } else {   // the PIR is built in non-private mode too (private-search.go:405)
    const uint64_t ebytes = g->dim * 4 + g->m * 4, E = ebytes / 8;
    std::vector<uint64_t> raw(g->n * E);
    for (uint64_t i = 0; i < g->n; ++i) {
      uint8_t* e = (uint8_t*)&raw[i * E];
      memcpy(e, &g->vectors[i * g->dim], g->dim * 4);
      memcpy(e + g->dim * 4, &g->graph[i * g->m], g->m * 4);
    }
    delete g->pir; g->pir = nullptr;
    CHK(pm_batchpir_create_shard(g->ctx, g->n, ebytes, g->m, raw.data(), 8, g->pir_seed, g->shard, g->nshards,
                                 &g->pir));
    g->pir->e.pf_off = g->dim * 4;   // the search reads the neighbour lists of the rows
    g->pir->e.pf_len = g->m * 4;
    if (g->skipPrep) CHK(pm_batchpir_dummy_preprocessing(g->pir));
    else CHK(pm_batchpir_preprocessing(g->pir));
  }
  const uint64_t target = (uint64_t)std::sqrt((double)g->n);
  std::unordered_map<uint64_t, bool> added;
  g->start.clear();
  for (uint64_t i = 0; i < target; ++i) {
    uint64_t x = g->rng.intn(g->n);
    while (added.count(x)) x = g->rng.intn(g->n);
    added[x] = true;
    g->start.push_back(x);
  }
  std::vector<uint32_t> ids(g->start.begin(), g->start.end());
  CHK(g->dstart.reserve(std::max<size_t>(4, ids.size() * 4)));
  if (!ids.empty()) HIPCHK(hipMemcpy(g->dstart.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice));
  if (!g->dvec->p && !g->nonprivate) {   // the start set's vectors themselves (GetStartVertex, non-private)
    const uint64_t ns = g->start.size();
    CHK(g->dstartvec.reserve(std::max<uint64_t>(4, ns * g->dim * 4)));
    if (g->synth) {
      DevBuf did;
      CHK(did.reserve(std::max<uint64_t>(8, ns * 8)));
      HIPCHK(hipMemcpy(did.p, g->start.data(), ns * 8, hipMemcpyHostToDevice));
      pmk::graph_synth_vecs(g->ctx->stream, did.as<uint64_t>(), ns, (uint32_t)g->dim, g->data_seed,
                            g->dstartvec.as<float>());
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(g->ctx->stream));
    } else {
      std::vector<float> sv(ns * g->dim);
      for (uint64_t i = 0; i < ns; ++i) memcpy(&sv[i * g->dim], g->vectors + g->start[i] * g->dim, g->dim * 4);
      if (ns) HIPCHK(hipMemcpy(g->dstartvec.p, sv.data(), sv.size() * 4, hipMemcpyHostToDevice));
    }
  }
  return 0;
}

// container/heap (Go stdlib) restated: up / down / Push / Pop on a min-heap.
static void heap_up(std::vector<VD>& h, int64_t j) {
  for (;;) { int64_t i = (j - 1) / 2; if (i == j || !(h[j].dist < h[i].dist)) break; std::swap(h[i], h[j]); j = i; }
}
static void heap_down(std::vector<VD>& h, int64_t i0, int64_t n) {
  int64_t i = i0;
  for (;;) {
    int64_t j1 = 2 * i + 1; if (j1 >= n || j1 < 0) break;
    int64_t j = j1, j2 = j1 + 1;
    if (j2 < n && h[j2].dist < h[j1].dist) j = j2;
    if (!(h[j].dist < h[i].dist)) break;
    std::swap(h[i], h[j]); i = j;
  }
}
static void heap_push(std::vector<VD>& h, VD x) { h.push_back(x); heap_up(h, (int64_t)h.size() - 1); }
static VD heap_pop(std::vector<VD>& h) {
  int64_t n = (int64_t)h.size() - 1; std::swap(h[0], h[n]); heap_down(h, 0, n);
  VD r = h.back(); h.pop_back(); return r;
}

// GetVertexInfo (private-search.go:441-506) for g->batch, with the L2 distance
// of every returned vector to the resident query computed on the GPU next to
// the decode (k_answer).  Fills g->nb and g->dist.  In two halves around the
// batch-PIR step, so that several sessions' steps can share one launch
// (pm_search_loop_batched): gvi_pre buckets the ids into this session's
// sub-queries (*fast: they are ready for a shared step; otherwise the step
// has already been served on this session's own stream), gvi_post maps the
// published rows back and parses them.
static int gvi_nonprivate(pm_graph* g, bool with_q) {
  const uint64_t n = g->batch.size(), m = g->m;
  for (uint64_t i = 0; i < n; ++i)
    memcpy(&g->nb[i * m], &g->graph[(uint64_t)g->batch[i] * m], m * 4);
  if (with_q && n) {
    hipStream_t st = g->ctx->stream;
    std::vector<uint32_t> u(g->batch.begin(), g->batch.end());
    CHK(g->dids.reserve(n * 4)); CHK(g->ddist.reserve(n * 4));
    HIPCHK(hipMemcpyAsync(g->dids.p, u.data(), n * 4, hipMemcpyHostToDevice, st));
    g->ctx->timed("l2_rows", (double)n * g->dim * 4, [&] {
      pmk::l2_rows(st, g->dvec->as<float>(), g->dim, n, g->dids.as<uint32_t>(), g->qdev(), (uint32_t)g->dim, g->ddist.as<float>());
    });
    HIPCHK(hipMemcpyAsync(g->dist.data(), g->ddist.p, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  return 0;
}
static int gvi_pre(pm_graph* g, bool with_q, bool* fast) {
  const uint64_t n = g->batch.size(), m = g->m;
  g->total += n;
  g->nb.resize(n * m);
  g->dist.assign(n, 0.0f);
  *fast = false;
  if (g->nonprivate) return gvi_nonprivate(g, with_q);
  Engine* e = &g->pir->e;
  // the ground-truth rows of the success check (private-search.go:483-497) are
  // pulled into the cache while the GPU answers
  for (uint64_t i = 0; g->graph && i < n; ++i) {
    const char* gr = (const char*)&g->graph[(uint64_t)g->batch[i] * m];
    for (uint64_t b = 0; b < m * 4; b += 64) __builtin_prefetch(gr + b);
    __builtin_prefetch(gr + m * 4 - 1);
  }
  g->qids.assign(g->batch.begin(), g->batch.end());
  g->rowp.resize(n);
  auto t = Clock::now();
  e->rows_partial = true;   // Entry2VectorAndNeighbors reads the neighbour list (the distance is in the header)
  CHK(bq_prepare(e, g->qids.data(), n, fast));
  if (!*fast)   // a partition at its query budget: the general path, served now
    CHK(batch_query_impl(e, g->qids.data(), n, nullptr, with_q ? g->qdev() : nullptr, (uint32_t)g->dim,
                         with_q ? g->dist.data() : nullptr, g->rowp.data(), nullptr));
  e->ctx->host_add(HT_BATCH_QUERY, ms_since(t));
  return 0;
}
static int gvi_post(pm_graph* g, bool with_q, bool fast) {
  if (g->nonprivate) return 0;
  const uint64_t n = g->batch.size(), m = g->m;
  Engine* e = &g->pir->e;
  if (fast) {
    auto t = Clock::now();
    bq_emit_fast(e, g->qids.data(), n, nullptr, with_q ? g->dist.data() : nullptr, g->rowp.data(), nullptr);
    CHK(bq_tail(e, n));
    e->ctx->host_add(HT_BATCH_QUERY, ms_since(t));
  }
  auto t_parse = Clock::now();
  const uint64_t nb_off = g->dim * 4;   // Entry2VectorAndNeighbors (private-search.go:418-439)
  for (uint64_t i = 0; i < n; ++i) {
    const char* r = (const char*)g->rowp[i] + nb_off;
    for (uint64_t b = 0; b < m * 4; b += 64) __builtin_prefetch(r + b);
  }
  uint32_t tmp[64];
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t* nbi = &g->nb[i * m];
    memcpy(nbi, (const char*)g->rowp[i] + nb_off, m * 4);
    if (memcmp(nbi, g->true_nb((uint64_t)g->batch[i], tmp), m * 4) == 0) g->succ++;
  }
  e->rows_partial = false;
  g->ctx->host_add(HT_GVI_PARSE, ms_since(t_parse));
  return 0;
}
static int get_vertex_info(pm_graph* g, bool with_q) {
  if (g->nshards > 1) return fail(PM_EINVAL, "a sharded graph searches through pm_search_loop_sharded (the shards' combine)");
  bool fast = false;
  CHK(gvi_pre(g, with_q, &fast));
  if (fast) {
    Engine* e = &g->pir->e;
    auto t = Clock::now();
    CHK(engine_step(e, with_q ? g->qdev() : nullptr, (uint32_t)g->dim));
    e->ctx->host_add(HT_BATCH_QUERY, ms_since(t));
  }
  return gvi_post(g, with_q, fast);
}

// ---- the GetGraphInfo plugin surface (graphann/search.go:20-25) ----------
// PIRGraphInfo's methods (private-search.go:441-531) as batch calls, so a
// caller that keeps its own beam search (graphann.SearchKNN in Go) still gets
// the private fetch, the decode and the L2 on the GPU.
extern "C" int pm_graph_get_metadata(pm_graph* g, uint64_t* n, uint64_t* dim, uint64_t* m) {
  if (!g) return fail(PM_EINVAL, "NULL argument");
  if (n) *n = g->n;
  if (dim) *dim = g->dim;
  if (m) *m = g->m;
  return 0;
}

extern "C" int pm_graph_get_vertex_info(pm_graph* g, const uint64_t* ids, uint64_t n, float* vecs, uint32_t* nbrs,
                                        uint8_t* ok, const float* query, float* dist) {
  if (!g || (n && !ids)) return fail(PM_EINVAL, "NULL argument");
  CHK(check_session(g));
  if (dist && !query) return fail(PM_EINVAL, "dist needs a query");
  if (g->nshards > 1) return fail(PM_EINVAL, "a sharded graph searches through pm_search_loop_sharded (the shards' combine)");
  if (!g->nonprivate && !g->pir) return fail(PM_EINVAL, "graph not preprocessed");
  for (uint64_t i = 0; i < n; ++i)
    if (ids[i] >= g->n) return fail(PM_EINVAL, "vertex id " + std::to_string(ids[i]) + " out of range");
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(g->ctx->device));
  if (query) HIPCHK(hipMemcpy(g->dq.p, query, g->dim * 4, hipMemcpyHostToDevice));
  const uint64_t dim = g->dim, m = g->m;
  uint32_t tmp[64];
  g->total += n;   // totalQueryNum (:443)
  if (g->nonprivate) {   // :445-455, BasicGraphInfo-style direct access
    for (uint64_t i = 0; i < n; ++i) {
      if (vecs) {
        if (g->synth) for (uint64_t j = 0; j < dim; ++j) vecs[i * dim + j] = graph_synth_vec(sm64(g->data_seed + DOM_SYNTH_VEC), ids[i], (uint32_t)dim, (uint32_t)j);
        else memcpy(vecs + i * dim, g->vectors + ids[i] * dim, dim * 4);
      }
      if (nbrs) memcpy(nbrs + i * m, g->true_nb(ids[i], tmp), m * 4);
      if (ok) ok[i] = 1;
    }
    if (dist) {
      g->batch.assign(ids, ids + n);
      g->nb.resize(n * m);
      g->dist.assign(n, 0.0f);
      CHK(gvi_nonprivate(g, true));
      memcpy(dist, g->dist.data(), n * 4);
    }
    return 0;
  }
  Engine* e = &g->pir->e;
  g->rowp.resize(n);
  std::vector<uint8_t> okv(n);
  std::vector<float> dv(n);
  e->rows_partial = false;   // whole rows: the caller reads the vectors too
  CHK(batch_query(e, ids, n, nullptr, query ? g->qdev() : nullptr, (uint32_t)dim, query ? dv.data() : nullptr,
                  g->rowp.data(), okv.data()));
  for (uint64_t i = 0; i < n; ++i) {   // Entry2VectorAndNeighbors (:418-439) + the success count (:483-497)
    const char* r = (const char*)g->rowp[i];
    if (vecs) memcpy(vecs + i * dim, r, dim * 4);
    if (nbrs) memcpy(nbrs + i * m, r + dim * 4, m * 4);
    if (memcmp(r + dim * 4, g->true_nb(ids[i], tmp), m * 4) == 0) g->succ++;
    if (ok) ok[i] = okv[i];
    if (dist) dist[i] = dv[i];
  }
  return 0;
}

extern "C" int pm_graph_get_start_vertex(pm_graph* g, uint64_t cap, uint64_t* ids, float* vecs, uint32_t* nbrs,
                                         uint64_t* count) {
  if (!g) return fail(PM_EINVAL, "NULL argument");
  if (!g->nonprivate && !g->pir) return fail(PM_EINVAL, "graph not preprocessed");
  const uint64_t ns = g->start.size(), dim = g->dim, m = g->m;
  if (count) *count = ns;
  uint32_t tmp[64];
  const uint64_t kv = sm64(g->data_seed + DOM_SYNTH_VEC);
  for (uint64_t i = 0; i < ns && i < cap; ++i) {   // non-private (:508-531)
    const uint64_t x = g->start[i];
    if (ids) ids[i] = x;
    if (vecs) {
      if (g->synth) for (uint64_t j = 0; j < dim; ++j) vecs[i * dim + j] = graph_synth_vec(kv, x, (uint32_t)dim, (uint32_t)j);
      else memcpy(vecs + i * dim, g->vectors + x * dim, dim * 4);
    }
    if (nbrs) memcpy(nbrs + i * m, g->true_nb(x, tmp), m * 4);
  }
  return 0;
}

// SearchKNN (graphann/search.go:114-234).  Same tie rules as oracle/pm_oracle.cpp.
static int search_knn_impl(pm_graph* g, const float* query, int k, int max_step, int parallel,
                           int benchmarking, int64_t* ids_out, int64_t* steps_out);
extern "C" int pm_search_knn(pm_graph* g, const float* query, int k, int max_step, int parallel,
                             int benchmarking, int64_t* ids_out, int64_t* steps_out) {
  if (g) CHK(check_session(g));
  auto t = Clock::now();
  int r = search_knn_impl(g, query, k, max_step, parallel, benchmarking, ids_out, steps_out);
  g->ctx->host_add(HT_SEARCH_KNN, ms_since(t));
  return r;
}
// SearchKNN in parts (the loop of search_knn_impl; pm_search_loop_batched
// interleaves them across sessions):
//   knn_begin  reset; unless benchmarking, the start set's distances to the
//              query (GPU, k_l2_rows) and the first `parallel` of them on the heap;
//   knn_batch  the ids of one step (search.go:150-172);
//   knn_update the returned vertices with a non-empty neighbour list become
//              known (search.go:185-218);
//   knn_end    top k by (dist, id) (search.go:222-233).
static void knn_add_known(pm_graph* g, int64_t id, const uint32_t* nb, float d, int64_t reach) {
  const uint64_t m = g->m;
  const uint32_t slot = (uint32_t)g->known_id.size();
  g->known.put((uint64_t)id, slot);
  g->known_nb.insert(g->known_nb.end(), nb, nb + m);
  g->known_dist.push_back(d);
  g->known_id.push_back(id);
  g->known_reach.push_back(reach);
}
// first half: reset + enqueue the start-set distances (async on the session's
// stream); knn_begin_finish completes it after the stream is synchronised
static void knn_reset(pm_graph* g) {
  g->known.clear();
  g->known_nb.clear(); g->known_dist.clear(); g->known_id.clear(); g->known_reach.clear();
  g->heap.clear();
}
static int knn_begin_enqueue(pm_graph* g, const float* query, int benchmarking) {
  if (!g->pir && !g->nonprivate) return fail(PM_EINVAL, "pm_graph_preprocess not called");
  hipStream_t st = g->ctx->stream;
  knn_reset(g);
  if (benchmarking) return 0;
  g->t_init = Clock::now();
  // the query stays resident for every distance this search computes; it and
  // the start-vertex distances move through pinned staging (async, no bounce)
  const uint64_t ns = g->start.size();
  CHK(g->stage_h.reserve(g->dim * 4 + ns * 4));
  float* qh = g->stage_h.as<float>();
  memcpy(qh, query, g->dim * 4);
  HIPCHK(hipMemcpyAsync(g->dq.p, qh, g->dim * 4, hipMemcpyHostToDevice, st));
  if (ns) {
    CHK(g->ddist.reserve(ns * 4));
    const bool ids = g->dvec->p != nullptr;   // all vectors on the device, or the start set's own (sharded / synthetic)
    g->ctx->timed("l2_rows", (double)ns * g->dim * 4, [&] {
      pmk::l2_rows(st, ids ? g->dvec->as<float>() : g->dstartvec.as<float>(), g->dim, ns,
                   ids ? g->dstart.as<uint32_t>() : nullptr, g->dq.as<float>(), (uint32_t)g->dim, g->ddist.as<float>());
    });
    HIPCHK(hipMemcpyAsync(qh + g->dim, g->ddist.p, ns * 4, hipMemcpyDeviceToHost, st));
  }
  return 0;
}
// sdh: the start set's distances (null: where knn_begin_enqueue put them)
static void knn_begin_finish(pm_graph* g, int parallel, int benchmarking, const float* sdh = nullptr) {
  if (benchmarking) return;
  const uint64_t ns = g->start.size();
  if (!sdh) sdh = g->stage_h.as<float>() + g->dim;
  // the first `parallel` start vertices in stable distance order (search.go:130-146):
  // a partial sort on (dist, position) selects exactly those
  g->fs.clear();
  for (uint64_t i = 0; i < ns; ++i) g->fs.push_back({{sdh[i], (int64_t)g->start[i]}, (uint32_t)i});
  const size_t take = std::min<size_t>(g->fs.size(), (size_t)std::max(parallel, 0));
  std::partial_sort(g->fs.begin(), g->fs.begin() + take, g->fs.end(), [](const auto& a, const auto& b) {
    return a.first.dist < b.first.dist || (a.first.dist == b.first.dist && a.second < b.second); });
  g->fs.resize(take);   // start ids are distinct: none of the first `parallel` is skipped as known
  g->ctx->host_add(HT_KNN_INIT, ms_since(g->t_init));
  for (size_t i = 0; (int64_t)g->heap.size() < parallel && i < g->fs.size(); ++i) {
    const int64_t id = g->fs[i].first.id;
    if (g->known.find((uint64_t)id)) continue;
    uint32_t tmp[64];   // GetStartVertex returns the start vertices' neighbour lists (non-private)
    knn_add_known(g, id, g->true_nb((uint64_t)id, tmp), g->fs[i].first.dist, 0);
    heap_push(g->heap, g->fs[i].first);
  }
}
static void knn_batch(pm_graph* g, int parallel, int benchmarking) {
  auto t_batch = Clock::now();
  const uint64_t m = g->m, n = g->n;
  g->batch.clear();
  for (int r = 0; r < parallel; ++r) {
    if (g->heap.empty() || benchmarking) {
      for (uint64_t i = 0; i < m; ++i) g->batch.push_back((int64_t)g->rng.intn(n));
    } else {
      const VD it = heap_pop(g->heap);
      const uint32_t* nb = &g->known_nb[(size_t)*g->known.find((uint64_t)it.id) * m];
      for (uint64_t i = 0; i < m; ++i) g->batch.push_back((int64_t)nb[i]);
    }
  }
  g->ctx->host_add(HT_KNN_BATCH, ms_since(t_batch));
}
static void knn_update(pm_graph* g, int step) {
  auto t_round = Clock::now();
  const uint64_t m = g->m;
  for (size_t i = 0; i < g->batch.size(); ++i) g->known.prefetch((uint64_t)g->batch[i]);
  if (g->known_id.capacity() < 4096) {   // a search keeps ~2,000 known vertices (20 steps x 96 ids)
    g->known_id.reserve(4096); g->known_dist.reserve(4096); g->known_reach.reserve(4096);
    g->known_nb.reserve(4096 * m);
  }
  for (size_t i = 0; i < g->batch.size(); ++i) {
    const int64_t id = g->batch[i];
    if (g->known.find((uint64_t)id)) continue;
    const uint32_t* nb = &g->nb[i * m];
    bool ok = false;
    for (uint64_t j = 0; j < m; ++j) if (nb[j] != 0) { ok = true; break; }
    if (!ok) continue;
    knn_add_known(g, id, nb, g->dist[i], step);
    heap_push(g->heap, {g->dist[i], id});
  }
  g->ctx->host_add(HT_KNN_UPDATE, ms_since(t_round));
}
static void knn_end(pm_graph* g, int k, int64_t* ids_out, int64_t* steps_out) {
  auto t_fin = Clock::now();
  g->all.clear();
  for (size_t i = 0; i < g->known_id.size(); ++i) g->all.push_back({g->known_dist[i], g->known_id[i]});
  // top k in (dist, id) order (search.go:222-233); ids are unique, so a partial sort is exact
  std::partial_sort(g->all.begin(), g->all.begin() + std::min<size_t>(g->all.size(), (size_t)std::max(k, 0)),
                    g->all.end(), [](const VD& a, const VD& b) {
    return a.dist < b.dist || (a.dist == b.dist && a.id < b.id); });
  for (int i = 0; i < k; ++i) {
    if (i >= (int)g->all.size()) { ids_out[i] = -1; if (steps_out) steps_out[i] = -1; }
    else { ids_out[i] = g->all[i].id; if (steps_out) steps_out[i] = g->known_reach[*g->known.find((uint64_t)g->all[i].id)]; }
  }
  g->ctx->host_add(HT_KNN_FINAL, ms_since(t_fin));
}
static int search_knn_impl(pm_graph* g, const float* query, int k, int max_step, int parallel,
                           int benchmarking, int64_t* ids_out, int64_t* steps_out) {
  CHK(knn_begin_enqueue(g, query, benchmarking));
  if (!benchmarking) HIPCHK(hipStreamSynchronize(g->ctx->stream));
  knn_begin_finish(g, parallel, benchmarking);
  for (int step = 0; step < max_step; ++step) {
    knn_batch(g, parallel, benchmarking);
    CHK(get_vertex_info(g, !benchmarking));
    if (benchmarking) continue;
    knn_update(g, step);
  }
  knn_end(g, k, ids_out, steps_out);
  return 0;
}

// GraphANNFrontend.SearchKNNBatch (graphann/search.go:236-245): SearchKNN of
// queries[i] for i = 0 .. nq-1 in order.  Defined as that loop over
// search_knn_impl (same ids, steps, counters and id stream afterwards); a
// non-private in-memory graph whose shape fits k_knn_batch (pm_knnb.hip) is
// searched on the device instead, one workgroup per query, a chunk of queries
// per launch.  A search draws from the id stream only where a pop finds its
// heap empty (search.go:155-159); the kernel flags such a query instead of
// answering it, and the flagged queries are re-run here in ascending order, so
// the stream is consumed exactly as by the loop.
extern "C" int pm_search_knn_batch(pm_graph* g, const float* queries, uint64_t nq, int k, int max_step, int parallel,
                                   int benchmarking, int64_t* ids, int64_t* steps, uint64_t* device_queries) {
  if (!g) return fail(PM_EINVAL, "NULL argument");
  CHK(check_session(g));
  if (device_queries) *device_queries = 0;
  if (nq && (!queries || !ids)) return fail(PM_EINVAL, "NULL argument");
  pm_ctx* c = g->ctx;
  const uint64_t dim = g->dim, m = g->m, ns = g->start.size(), kk = (uint64_t)std::max(k, 0);
  auto host_query = [&](uint64_t i) {
    return search_knn_impl(g, queries + i * dim, k, max_step, parallel, benchmarking, ids + i * kk,
                           steps ? steps + i * kk : nullptr);
  };
  bool dev = nq && g->nonprivate && !g->synth && g->nshards == 1 && !benchmarking && g->dvec->p && g->graph &&
             g->n < 0xffffffffull && k > 0 && max_step >= 0 && parallel > 0 &&
             pmk::knn_batch_ok(dim, m, ns, (uint64_t)max_step, (uint64_t)parallel);
  if (dev && g->graph_ids_ok < 0) {   // the kernel follows the graph's ids without a host in between
    g->graph_ids_ok = 1;
    for (uint64_t i = 0; i < g->n * m; ++i)
      if (g->graph[i] >= g->n) { g->graph_ids_ok = 0; break; }
  }
  if (!dev || !g->graph_ids_ok) {
    for (uint64_t i = 0; i < nq; ++i) CHK(host_query(i));
    return 0;
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  if (!g->dgraph->p) {   // the neighbour lists on the device, once per graph
    CHK(g->dgraph->reserve(g->n * m * 4));
    HIPCHK(hipMemcpy(g->dgraph->p, g->graph, g->n * m * 4, hipMemcpyHostToDevice));
  }
  const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>({nq, 1u << 15, (256ull << 20) / (kk * 16)}));
  std::vector<uint32_t> flags(nq);
  pmk::KnbArgs A{};
  A.vec = g->dvec->as<float>();
  A.graph = g->dgraph->as<uint32_t>();
  A.start = g->dstart.as<uint32_t>();
  A.ns = (uint32_t)ns; A.dim = (uint32_t)dim; A.m = (uint32_t)m; A.k = (uint32_t)k;
  A.max_step = (uint32_t)max_step; A.parallel = (uint32_t)parallel;
  A.kcap = pmk::knn_batch_kcap((uint64_t)parallel, (uint64_t)max_step, m);
  for (uint64_t q0 = 0; q0 < nq; q0 += chunk) {
    const uint64_t cn = std::min(chunk, nq - q0);
    CHK(g->kb_q.reserve(cn * dim * 4)); CHK(g->kb_ids.reserve(cn * kk * 8));
    CHK(g->kb_steps.reserve(cn * kk * 8)); CHK(g->kb_flags.reserve(cn * 4));
    HIPCHK(hipMemcpyAsync(g->kb_q.p, queries + q0 * dim, cn * dim * 4, hipMemcpyHostToDevice, st));
    A.queries = g->kb_q.as<float>(); A.nq = (uint32_t)cn;
    A.ids = g->kb_ids.as<int64_t>(); A.steps = g->kb_steps.as<int64_t>(); A.needs_host = g->kb_flags.as<uint32_t>();
    c->timed("knn_batch", (double)cn * (double)(ns + (uint64_t)max_step * parallel * m) * (double)(dim + m) * 4.0,
             [&] { pmk::knn_batch(st, A); });
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ids + q0 * kk, g->kb_ids.p, cn * kk * 8, hipMemcpyDeviceToHost, st));
    if (steps) HIPCHK(hipMemcpyAsync(steps + q0 * kk, g->kb_steps.p, cn * kk * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(flags.data() + q0, g->kb_flags.p, cn * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  uint64_t nhost = 0;
  for (uint64_t i = 0; i < nq; ++i) nhost += flags[i] != 0;
  g->total += (nq - nhost) * (uint64_t)max_step * (uint64_t)parallel * m;   // totalQueryNum of the device's queries
  if (device_queries) *device_queries = nq - nhost;
  if (nhost) {
    auto t = Clock::now();
    for (uint64_t i = 0; i < nq; ++i)
      if (flags[i]) CHK(host_query(i));
    c->host_add(HT_KNN_BATCH_FALLBACK, ms_since(t));
  }
  return 0;
}

// private-search.go:216-240
extern "C" int pm_search_loop(pm_graph* g, const float* queries, uint64_t q, int k, int step, int parallel,
                              int benchmarking, int64_t* answers, double* online_s, double* maint_s) {
  if (g) CHK(check_session(g));
  std::vector<int64_t> steps(k);
  double maint = 0;
  auto t0 = std::chrono::steady_clock::now();
  for (uint64_t i = 0; i < q; ++i) {
    CHK(pm_search_knn(g, queries + i * g->dim, k, step, parallel, benchmarking, answers + i * k, steps.data()));
    if (g->pir) {
      Engine* e = &g->pir->e;
      if (e->FBN + (uint64_t)step * (uint64_t)parallel + 10 >= e->Support) {
        auto a = std::chrono::steady_clock::now();
        CHK(batch_prep(e));
        maint += std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count();
      }
    }
  }
  double total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (online_s) *online_s = total - maint;
  if (maint_s) *maint_s = maint;
  return 0;
}

// S client sessions served concurrently on one GPU: session i runs the
// private-search.go:216-240 loop (search + its own maintenance trigger) over
// queries[i*q .. (i+1)*q) on its own host thread and stream.  The sessions'
// step kernels overlap each other's host work.  online_s / maint_s: S entries.
extern "C" int pm_search_loop_sessions(pm_graph** gs, uint32_t S, const float* queries, uint64_t q, int k,
                                       int step, int parallel, int64_t* answers, double* wall_s,
                                       double* online_s, double* maint_s) {
  if (!gs || !S || (!queries && q) || (!answers && q)) return fail(PM_EINVAL, "NULL argument");
  for (uint32_t i = 0; i < S; ++i)
    if (gs[i]) CHK(check_session(gs[i]));
  for (uint32_t i = 0; i < S; ++i) {
    if (!gs[i]) return fail(PM_EINVAL, "NULL session");
    for (uint32_t j = 0; j < i; ++j)
      if (gs[j] == gs[i] || gs[j]->ctx == gs[i]->ctx) return fail(PM_EINVAL, "sessions need distinct graphs and contexts");
  }
  std::vector<int> rc(S, 0);
  std::vector<std::string> msg(S);
  std::vector<double> on(S, 0.0), mt(S, 0.0);
  std::atomic<uint32_t> ready{0};
  std::atomic<bool> go{false};
  std::vector<std::thread> th;
  th.reserve(S);
  for (uint32_t i = 0; i < S; ++i) {
    th.emplace_back([&, i] {
      pm_graph* g = gs[i];
      if (hipSetDevice(g->ctx->device) != hipSuccess) { rc[i] = PM_EHIP; msg[i] = "hipSetDevice"; ready++; return; }
      ready++;
      while (!go.load(std::memory_order_acquire)) std::this_thread::yield();
      rc[i] = pm_search_loop(g, queries + i * q * g->dim, q, k, step, parallel, 0, answers + i * q * (uint64_t)k,
                             &on[i], &mt[i]);
      if (rc[i]) msg[i] = pm_last_error();
      else if (hipStreamSynchronize(g->ctx->stream) != hipSuccess) { rc[i] = PM_EHIP; msg[i] = "stream sync"; }
    });
  }
  while (ready.load() < S) std::this_thread::yield();
  auto t0 = std::chrono::steady_clock::now();
  go.store(true, std::memory_order_release);
  for (auto& t : th) t.join();
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (wall_s) *wall_s = wall;
  for (uint32_t i = 0; i < S; ++i) {
    if (online_s) online_s[i] = on[i];
    if (maint_s) maint_s[i] = mt[i];
  }
  for (uint32_t i = 0; i < S; ++i)
    if (rc[i]) return fail(rc[i], "session " + std::to_string(i) + ": " + msg[i]);
  return 0;
}

// ---------------------------------------------------------------------------
// Batched multi-session serving: S client sessions in
// lock-step, every batch-PIR round of all of them ONE step over S x 16
// partitions (k_match -> k_resolve -> [k_gather] -> k_answer), so a round
// costs one launch sequence for all clients instead of one per client.  Each
// session keeps its own keys, hint state, cache, counters, search state and
// maintenance; the shared step only concatenates their sub-queries (a
// session's partition p is the step's partition s * 16 + p) and scores each
// decoded row against its own session's query (PmPart::qv).  Host work (the
// sessions' searches) runs on a pool of worker threads between steps.
// ---------------------------------------------------------------------------
struct SpinBarrier {
  std::atomic<uint32_t> count{0}, gen{0};
  uint32_t n = 1;
  void wait() {
    const uint32_t g0 = gen.load(std::memory_order_acquire);
    if (count.fetch_add(1, std::memory_order_acq_rel) + 1 == n) {
      count.store(0, std::memory_order_relaxed);
      gen.fetch_add(1, std::memory_order_release);
    } else {
      while (gen.load(std::memory_order_acquire) == g0) std::this_thread::yield();
    }
  }
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
  DevBuf parts_d, done, prep_parts, desc_d, qset;
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

// The sharded loop's exchange: the caller's combine (an in-place SUM
// all-reduce of a team's records over the ranks, ordered on the given stream),
// issued in one global order (round-major, then team) on every rank so the
// ranks' collectives match; or model_peers: the partitions this rank does not
// hold are answered from the synthetic graph's spec on the device (a shard
// layout wider than the job, measured one shard per GPU).
struct ShardComb {
  pm_combine_fn fn = nullptr;   // include/pacmann.h
  void* user = nullptr;
  bool model_peers = false;
  uint32_t NG = 1;
  uint64_t* const* bufs = nullptr;   // the caller's device buffers, one per team (null: the library's)
  std::atomic<uint64_t> ticket{0};
  std::atomic<bool> abort{false};
};

static int group_upload_parts(StepGroup& G) {
  std::vector<PmPart> v;
  v.reserve((size_t)G.S * G.P);
  for (uint32_t s = 0; s < G.S; ++s) {
    Engine* e = G.es[s];
    for (uint32_t p : G.lp) {
      PmPart d = e->parts[p].d;
      d.qv = G.qv.empty() ? nullptr : G.qv[s];
      v.push_back(d);
    }
  }
  HIPCHK(hipMemcpyAsync(G.parts_d.p, v.data(), v.size() * sizeof(PmPart), hipMemcpyHostToDevice, G.c->stream));
  HIPCHK(hipStreamSynchronize(G.c->stream));
  G.gen.resize(G.S);
  for (uint32_t s = 0; s < G.S; ++s) G.gen[s] = G.es[s]->prep_gen;
  return 0;
}

// Common setup of a step group over clients of one server (same DB, shard
// and parameters): device buffers and the clients' parts.
static int group_init(StepGroup& G, pm_ctx* c) {
  G.c = c;
  G.S = (uint32_t)G.es.size();
  const Engine& e = *G.es[0];
  G.P = (uint32_t)e.P; G.maxPH = e.maxPH; G.ph8 = e.ph8; G.maxSS = e.maxSS; G.E = (uint32_t)e.E;
  G.lp = e.owned_list;
  G.Pl = (uint32_t)G.lp.size();
  HIPCHK(hipSetDevice(c->device));
  CHK(G.parts_d.reserve(std::max<size_t>(1, (size_t)G.S * G.Pl) * sizeof(PmPart)));
  CHK(G.done.reserve(4 * (3 + 65536)));
  const uint32_t init[3] = {1u << 31, 0, 0};
  HIPCHK(hipMemcpy(G.done.p, init, sizeof init, hipMemcpyHostToDevice));
  return group_upload_parts(G);
}

// Session s's sub-queries for the next shared step into its stage slot (the
// session's own task, after gvi_pre: the data is in this core's cache).  A
// session with more than `stride` sub-queries leaves its slot invalid and the
// step is built the general way (group_step raises the stride).
static void group_stage_session(StepGroup& G, uint32_t s) {
  StepGroup::SessStage& ss = G.stg[s];
  ss.ok = false;
  if (!G.stage_on || !G.stride) return;
  const Engine* e = G.es[s];
  PmSub* dst = G.stage_h.as<PmSub>() + (uint64_t)s * G.stride;
  uint32_t n = 0, nreal = 0, maxpp = 0, live = 0;
  double bytes = 0;
  ss.pc.resize(G.Pl);
  for (uint32_t li = 0; li < G.Pl; ++li) {
    const uint32_t p = G.lp[li], a = e->sb[p], b = e->sb[p + 1];
    if (n + (b - a) > G.stride) { ss.n = n + (b - a); return; }
    const double ab = answer_bytes(e->parts[p].d, G.E);
    for (uint32_t j = a; j < b; ++j) {
      PmSub x = e->subs[j];
      x.part = s * G.Pl + li;
      dst[n++] = x;
      if (x.kind == SUB_REAL || x.kind == SUB_DUMMY) bytes += ab;
      nreal += x.kind == SUB_REAL;
    }
    ss.pc[li] = b - a;
    maxpp = std::max(maxpp, b - a);
    live += b > a;
  }
  ss.n = n; ss.nreal = nreal; ss.maxpp = maxpp; ss.live = live; ss.bytes = bytes;
  ss.step = G.nstep;
  ss.ok = true;
}

// The kernels of one shared step whose descriptor S is complete: the hint
// search + resolution (k_match_resolve_s where the shapes hold), the split
// gather for wide sets, the answer; the completion event unless the records
// go to a combine.  (group_step; the device loop's steps, run_batched_dev.)
static int group_step_launch(StepGroup& G, PmStep& S, uint32_t max_per_part, uint32_t nreal, double ans_bytes) {
  pm_ctx* c = G.c;
  hipStream_t st = c->stream;
  const uint32_t nsub = S.nsub;
  StepBufs& B = G.buf;
  auto t0 = Clock::now();
  const bool lds = pmk::step_resolve_lds_ok(G.maxPH, max_per_part);
  S.nsplit = c->no_split ? 1 : pmk::step_gather_split(G.maxSS, nsub);
  const pmk::StepOpts opts = pmk::step_opts();   // one snapshot: np_live, the qset and the kernels agree
  if (pmk::step_qset_ok(S, opts, lds, G.ph8, G.maxPH, max_per_part, G.maxSS)) {
    S.qw = (G.maxSS + 7) & ~7u;
    CHK(G.qset.reserve((uint64_t)nsub * S.qw * 2));
    S.qset = G.qset.as<uint16_t>();
  }
  if (pmk::step_match_resolve_ok(S, opts, lds)) {   // one launch: match + resolve per partition
    if (pmk::step_match_resolve_small(opts, G.ph8, G.maxPH, max_per_part)) S.np_live = 0;   // resolvers do not count in
#ifdef PM_MR_STAMPS
    static const char* mr_file = getenv("PM_MR_STAMPS");   // append {np} + np x 8 stamps per step
    static std::atomic<int> mr_steps{0};   // the first 40 steps of the run
    const bool mr_this = mr_file && mr_steps.fetch_add(1) < 40;
    const uint64_t np = S.np;
    if (mr_this) {
      CHK(B.stamps.reserve(np * 8 * 8));
      HIPCHK(hipMemsetAsync(B.stamps.p, 0, np * 8 * 8, st));
      S.stamps = B.stamps.as<uint64_t>();
    }
#endif
    c->timed_ext("match_resolve", (double)nreal * G.maxPH, [&](pmk::PmEvents ev) { pmk::step_match_resolve(st, S, opts, G.ph8, G.maxPH, max_per_part, ev); }, 2);
#ifdef PM_MR_STAMPS
    if (mr_this) {
      CHK(dump_stamps(st, mr_file, &np, sizeof np, B.stamps, np * 8));
      S.stamps = nullptr;
    }
#endif
  } else {
    int path = 0;
    c->timed_ext("hint_match", (double)nreal * G.maxPH, [&](pmk::PmEvents ev) { path = pmk::step_match(st, S, opts, G.ph8, G.maxPH, max_per_part, ev); }, 2);
    c->count_match_path(path);
    c->timed_ext("resolve", 0, [&](pmk::PmEvents ev) { pmk::step_resolve(st, S, lds, ev); }, 2);
  }
  if (S.nsplit > 1) {
    CHK(B.part_x.reserve((uint64_t)nsub * S.nsplit * (G.E & ~3u) * 8));
    S.part_x = B.part_x.as<uint64_t>();
    c->timed_ext("gather", ans_bytes, [&](pmk::PmEvents ev) { pmk::step_gather(st, S, ev); }, 2);
  }
#ifdef PM_ANSWER_STAMPS
  static const char* stamp_file = getenv("PM_ANSWER_STAMPS");   // append {nsub} + nsub x 8 stamps per step
  static std::atomic<int> stamp_steps{0};   // the first 40 steps of the run (file size)
  const bool stamp_this = stamp_file && stamp_steps.fetch_add(1) < 40;
  if (stamp_this) {
    CHK(B.stamps.reserve((uint64_t)nsub * 8 * 8));
    HIPCHK(hipMemsetAsync(B.stamps.p, 0, (uint64_t)nsub * 8 * 8, st));
    S.stamps = B.stamps.as<uint64_t>();
  }
#endif
  c->timed_ext("answer", S.nsplit > 1 ? 0 : ans_bytes, [&](pmk::PmEvents ev) { pmk::step_answer(st, S, G.maxSS, ev); }, 2);
  if (!G.comb) G.seq = c->record_done(st);   // sharded: group_exchange publishes the records
  HIPCHK(hipGetLastError());
#ifdef PM_ANSWER_STAMPS
  if (stamp_this) {
    const uint64_t h = nsub;
    CHK(dump_stamps(st, stamp_file, &h, sizeof h, B.stamps, (uint64_t)nsub * 8));
  }
#endif
  c->host_add(HT_STEP_LAUNCH, ms_since(t0));
  G.pf_w0 = S.pf_w0; G.pf_w1 = S.pf_w1;
  return 0;
}

// One shared step over the clients whose sub-queries are ready (in[s]).
static int group_step(StepGroup& G, const std::vector<char>& in) {
  pm_ctx* c = G.c;
  hipStream_t st = c->stream;
  // timing 3: events on every kSampleSteps-th shared step of this stream (7: coprime
  // with the 20 rounds of a search, so every round position is sampled); the
  // events' dispatch-packet and completion handling cost ~5 % of the serving
  // rate when every launch carries them
  constexpr uint64_t kSampleSteps = 7;
  c->sample_now = c->sample_ctr++ % kSampleSteps == 0;
  bool stale = false;   // a client re-preprocessed since its parts were copied
  for (uint32_t s = 0; s < G.S; ++s) stale |= G.es[s]->prep_gen != G.gen[s];
  if (stale) CHK(group_upload_parts(G));
  G.sb.assign(1, 0);
  G.base.assign(G.S, 0);
  uint32_t max_per_part = 0, np_live = 0, nreal = 0, nsub = 0;
  double ans_bytes = 0;
  const uint32_t np = G.S * G.Pl;
  // the sessions' staged slots (group_stage_session), if every one is current
  bool staged = G.stage_on && G.stride > 0 && G.stg.size() == G.S;
  uint32_t need = 0;   // the largest session's sub-queries (the next stride)
  for (uint32_t s = 0; staged && s < G.S; ++s) {
    const StepGroup::SessStage& ss = G.stg[s];
    if (!in[s]) continue;
    need = std::max(need, ss.n);
    if (!ss.ok || ss.step != G.nstep) staged = false;
    nsub += ss.n;
  }
  if (staged && nsub <= kArgSubs && np <= kArgParts) staged = false;   // kernel-argument descriptors: the general way
  G.nstep++;
  PmSub* const stage = G.stage_h.as<PmSub>();
  if (staged) {   // compact the slots in place; the partition offsets follow the subs
    uint32_t off = 0;
    for (uint32_t s = 0; s < G.S; ++s) {
      const StepGroup::SessStage& ss = G.stg[s];
      G.base[s] = off;
      const uint32_t n = in[s] ? ss.n : 0;
      if (n && off != s * G.stride) memmove(stage + off, stage + (uint64_t)s * G.stride, (size_t)n * sizeof(PmSub));
      for (uint32_t li = 0; li < G.Pl; ++li) G.sb.push_back(G.sb.back() + (in[s] ? ss.pc[li] : 0));
      if (in[s]) {
        max_per_part = std::max(max_per_part, ss.maxpp);
        np_live += ss.live;
        ans_bytes += ss.bytes;
        nreal += ss.nreal;
      }
      off += n;
    }
  } else {
    G.subs.clear();
    for (uint32_t s = 0; s < G.S; ++s) {
      Engine* e = G.es[s];
      G.base[s] = (uint32_t)G.subs.size();
      for (uint32_t li = 0; li < G.Pl; ++li) {
        const uint32_t p = G.lp[li];
        if (in[s]) {
          for (uint32_t j = e->sb[p]; j < e->sb[p + 1]; ++j) {
            PmSub x = e->subs[j];
            x.part = s * G.Pl + li;
            G.subs.push_back(x);
            if (x.kind == SUB_REAL || x.kind == SUB_DUMMY) ans_bytes += answer_bytes(e->parts[p].d, G.E);
            nreal += x.kind == SUB_REAL;
          }
          const uint32_t n = e->sb[p + 1] - e->sb[p];
          max_per_part = std::max(max_per_part, n);
          np_live += n > 0;
        }
        G.sb.push_back((uint32_t)G.subs.size());
      }
      need = std::max(need, in[s] ? (uint32_t)G.subs.size() - G.base[s] : 0u);
    }
    nsub = (uint32_t)G.subs.size();
  }
  G.nsub = nsub;
  if (G.stage_on && need > G.stride) {   // slots for the next step's staging (the tasks write them after this step)
    G.stride = (need + 7) & ~7u;
    CHK(G.stage_h.reserve((size_t)G.S * G.stride * sizeof(PmSub) + (size_t)(np + 1) * 4));
    if (G.stg.size() != G.S) G.stg.resize(G.S);
  }
  if (nsub == 0) return 0;
  const uint32_t words = (G.maxPH + 63) / 64, cblk = pmk::step_match_blocks(G.maxPH);
  StepBufs& B = G.buf;
  CHK(B.reserve(nsub, np, words, cblk, G.E));
  const size_t dsub = nsub * sizeof(PmSub);
  char* dh;
  if (staged) {   // the compacted slots are the descriptor; the offsets right after them
    dh = G.stage_h.as<char>();
    memcpy(dh + dsub, G.sb.data(), (np + 1) * 4);
  } else {
    CHK(B.desc_h.reserve(dsub + (np + 1) * 4));
    dh = B.desc_h.as<char>();
    memcpy(dh, G.subs.data(), dsub);
    memcpy(dh + dsub, G.sb.data(), (np + 1) * 4);
  }
  PmStep S{};
  S.parts = G.parts_d.as<PmPart>();
  S.subs_h = (const PmSub*)dh;
  S.sb_h = (const uint32_t*)(dh + dsub);
  B.fill(S, words, cblk);
  if (!(nsub <= kArgSubs && np <= kArgParts)) {
    // a large descriptor crosses PCIe once, by DMA, instead of as thousands of
    // zero-copy reads by the match workgroups; k_match* stage it from here
    CHK(G.desc_d.reserve(dsub + (np + 1) * 4));
    HIPCHK(hipMemcpyAsync(G.desc_d.p, dh, dsub + (np + 1) * 4, hipMemcpyHostToDevice, st));
    S.subs_h = G.desc_d.as<PmSub>();
    S.sb_h = (const uint32_t*)(G.desc_d.as<char>() + dsub);
    S.subs = const_cast<PmSub*>(S.subs_h);   // the DMA'd descriptor is the device copy
    S.sb = const_cast<uint32_t*>(S.sb_h);
  }
  S.done = G.done.as<uint32_t>();
  Engine* e0 = G.es[0];
  S.db = e0->db->as<uint64_t>();
  S.q = nullptr;   // each partition's PmPart::qv
  if (G.comb) {   // sharded: results stay on the device for group_exchange's records
    CHK(G.out_d.reserve(step_out_bytes(nsub, G.E)));
    step_out(S, G.out_d.p, nsub);
  } else {
    CHK(B.out_h.reserve(step_out_bytes(nsub, G.E)));
    step_out(S, B.out_h.p, nsub);
  }
  S.E = G.E; S.dim = G.dim; S.nsub = nsub; S.np = np;
  S.np_live = np_live;
  S.args_valid = (nsub <= kArgSubs && np <= kArgParts) ? 1u : 0u;
  if (S.args_valid) {   // (never the staged form)
    memcpy(S.subs_a, G.subs.data(), dsub);
    memcpy(S.sb_a, G.sb.data(), (np + 1) * 4);
  }
  S.token = next_token(G.token);
  step_read_window(S, e0->pf_off, e0->pf_len, G.E);
  S.rows_partial = host_rows_partial(c, G.rows_partial);
  return group_step_launch(G, S, max_per_part, nreal, ans_bytes);
}

// The lines session s's collect will read (its result headers and the row
// words the host reads, its localCache slots, its ids' ground-truth rows),
// requested one task ahead by the worker that will most likely take it: the
// misses then resolve while the worker serves the session before it.
static void prefetch_session(StepGroup& G, uint32_t s, const pm_graph* g) {
  const Engine* e = G.es[s];
  const uint32_t n = (uint32_t)e->subs.size();
  const PmOutHdr* hdr = G.buf.out_h.as<PmOutHdr>() + G.base[s];
  const char* rows = G.buf.out_h.as<char>() + (size_t)G.nsub * sizeof(PmOutHdr) + (size_t)G.base[s] * G.E * 8;
  for (uint32_t j = 0; j < n; j += 2) __builtin_prefetch(hdr + j);
  for (uint32_t j = 0; j < n; ++j)
    for (uint32_t w = G.pf_w0; w < G.pf_w1; w += 8) __builtin_prefetch(rows + ((size_t)j * G.E + w) * 8);
  // (not its localCache slots: that session's collect may be rehashing its
  // FlatMap on another worker right now; group_collect prefetches them itself)
  if (g->graph)
    for (size_t b = 0; b < g->batch.size(); ++b) __builtin_prefetch(&g->graph[(uint64_t)g->batch[b] * g->m]);
}

// Session s's share of the last shared step: wait for its results (tokens and
// row checksums, polled by the session's own worker, so a team checks its
// sub-queries in parallel) and update its host mirrors.
static int group_collect(StepGroup& G, uint32_t s) {
  Engine* e = G.es[s];
  const uint32_t n = (uint32_t)e->subs.size();
  for (uint32_t j = 0; j < n; ++j)   // the localCache slots post_results fills, requested ahead
    if (e->subs[j].kind == SUB_REAL) e->parts[e->subs[j].part].cache.prefetch(e->subs[j].idx);
  PmOutHdr* hdr = G.buf.out_h.as<PmOutHdr>();
  uint64_t* rows = (uint64_t*)(G.buf.out_h.as<char>() + (size_t)G.nsub * sizeof(PmOutHdr));
  auto t_wait = Clock::now();
  CHK(wait_step(e->ctx, hdr + G.base[s], n, G.token, (const char*)(rows + (uint64_t)G.base[s] * G.E),
                (size_t)G.E * 8, (size_t)G.pf_w0 * 8, (size_t)(G.pf_w1 - G.pf_w0) * 8, G.seq, G.c));
  e->ctx->host_add(HT_STEP_WAIT, ms_since(t_wait));
  auto tp = Clock::now();
  post_results(e, hdr, rows, n, G.base[s], G.token);
  e->ctx->host_add(HT_STEP_POST, ms_since(tp));
  return 0;
}

// The team's queries (staged in G.qstage) to the device and every session's
// start-set distances (search.go:130-146) in one k_l2_rows launch: over the
// device copy of all vectors by start id, or (sharded / synthetic graphs)
// over the sessions' start vectors themselves.
static int group_start_dist(StepGroup& G, pm_graph** gs) {
  hipStream_t st = G.c->stream;
  float* qst = G.qstage.as<float>();
  HIPCHK(hipMemcpyAsync(G.qbuf.p, qst, (uint64_t)G.S * G.dim * 4, hipMemcpyHostToDevice, st));
  const uint64_t nrows = (uint64_t)G.S * G.ns;
  if (nrows) {
    const bool ids = gs[0]->dvec->p != nullptr;
    G.c->timed("l2_rows", (double)nrows * G.dim * 4, [&] {
      pmk::l2_rows(st, ids ? gs[0]->dvec->as<float>() : G.start_vec.as<float>(), G.dim, nrows,
                   ids ? G.start_ids.as<uint32_t>() : nullptr, G.qbuf.as<float>(), G.dim, G.start_dist.as<float>(),
                   G.ns);
    });
    HIPCHK(hipMemcpyAsync(qst + (uint64_t)G.S * G.dim, G.start_dist.p, nrows * 4, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// SimpleBatchPianoPIR.Preprocessing (batch-pir.go:119-155) of the clients
// `who` (batch PIR engines of one server: same DB and parameters, partitions
// lp), as ONE launch set over all their partitions on c's stream, with its
// parts staged in pbuf.  Each client's maintenance time is the set's wall time
// (added to *mt[i] when given).
// Async form (stage non-null): the parts go up from the pinned `stage` (its
// previous copy waited for through *stage_ev), nothing waits for the launch
// set, and the caller times it with events (mt unused).
static int prep_clients(pm_ctx* c, DevBuf& pbuf, const std::vector<uint32_t>& lp, const std::vector<Engine*>& who,
                        const std::vector<double*>* mt, HostBuf* stage = nullptr, hipEvent_t* stage_ev = nullptr) {
  if (who.empty()) return 0;
  auto t0 = Clock::now();
  std::vector<PmPart> hp;
  std::vector<uint64_t> todo;
  for (Engine* e : who) {
    e->FBN = 0; e->QMIP = 0;
    CHK(engine_prep_host(e, 0, e->P, todo, c->stream));   // ordered before the launch set below
  }
  // partition-major: the clients' folds of one partition run side by side and
  // share its DB rows through the caches instead of re-reading them per client
  for (uint32_t p : lp)
    for (Engine* e : who) hp.push_back(e->parts[p].d);
  const Engine* e0 = who[0];
  bool skip = false;
  for (Engine* e : who) skip |= e->skipPrep != e0->skipPrep;
  if (skip) return fail(PM_EINVAL, "batched sessions mix Preprocessing and DummyPreprocessing");
  CHK(pbuf.reserve(hp.size() * sizeof(PmPart)));
  if (stage) {
    if (*stage_ev) HIPCHK(hipEventSynchronize(*stage_ev));
    else HIPCHK(hipEventCreateWithFlags(stage_ev, hipEventDisableTiming));
    CHK(stage->reserve(hp.size() * sizeof(PmPart)));
    memcpy(stage->p, hp.data(), hp.size() * sizeof(PmPart));
    HIPCHK(hipMemcpyAsync(pbuf.p, stage->p, hp.size() * sizeof(PmPart), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(*stage_ev, c->stream));
  } else {
    HIPCHK(hipMemcpyAsync(pbuf.p, hp.data(), hp.size() * sizeof(PmPart), hipMemcpyHostToDevice, c->stream));
  }
  CHK(engine_prep_launch(c, e0, pbuf.as<PmPart>(), (int)hp.size(), hp.data(), (uint32_t)who.size(), !stage));
  c->host_add(HT_PREP_SETS, (double)who.size());
  const double t = std::chrono::duration<double>(Clock::now() - t0).count();
  for (size_t i = 0; i < who.size(); ++i) {
    who[i]->prepCount++;
    record_stats(who[i], t);
    if (mt) *(*mt)[i] += t;
  }
  return 0;
}
// The clients of team G with need[s], as one launch set on the team's stream.
static int group_prep(StepGroup& G, const std::vector<char>& need, std::vector<double>* mt) {
  std::vector<Engine*> who;
  std::vector<double*> mts;
  for (uint32_t s = 0; s < G.S; ++s)
    if (need[s]) {
      who.push_back(G.es[s]);
      if (mt) mts.push_back(&(*mt)[s]);
    }
  return prep_clients(G.c, G.prep_parts, G.lp, who, mt ? &mts : nullptr);
}

// ---- sharded private search (pm_search_loop_sharded) --------------------
// Every rank runs the same sessions (same seeds, same queries) over its shard
// of the graph DB.  A round: each session's GetVertexInfo batch is bucketed
// (bq_prepare: the global decisions, identical on every rank) and its
// sub-queries on this rank's partitions join the team's shared step; the step's
// answers become per-id records [session][position] = {neighbour words, dist |
// ok << 32}, zero where this rank holds no answer; ONE combine per shared step
// sums the records over the ranks; every rank then reads all records back and
// continues the identical searches.  Host mirrors (FinishedQueryNum, the local
// cache, counters, the maintenance trigger) are per rank and per partition, as
// in the single-rank engine, so each rank's partitions evolve exactly as the
// unsharded engine's do.

// Bucket session s's batch (rank-local sub-queries) and fill its rows of the
// record map: the answering sub-query (client-local index) of each position,
// -1 (no local answer) or -2 (answered by a modelled peer).  A batch that
// needs several steps here (a partition at its query budget) is served now on
// the session's own stream and its records packed on the host.
static int gvi_pre_sharded(pm_graph* g, StepGroup& G, uint32_t s, bool* fast) {
  const uint64_t n = g->batch.size(), m = g->m;
  if (n != G.npos) return fail(PM_EINVAL, "sharded search: every round must fetch parallel * m ids");
  g->total += n;
  g->nb.resize(n * m);
  g->dist.assign(n, 0.0f);
  Engine* e = &g->pir->e;
  g->qids.assign(g->batch.begin(), g->batch.end());
  auto t = Clock::now();
  e->rows_partial = true;
  CHK(bq_prepare(e, g->qids.data(), n, fast));
  int32_t* map = G.map_h.as<int32_t>() + (uint64_t)s * G.npos;
  if (*fast) {
    e->resp_map.clear();
    for (size_t j = 0; j < e->subs.size(); ++j) {
      const uint32_t k = e->subs[j].kind;
      if (k == SUB_REAL || k == SUB_HOSTCACHE) e->resp_map.put(e->sub_gid[j], (uint32_t)j);   // last wins
    }
  } else {
    g->rowp.resize(n);
    g->okv.assign(n, 0);
    CHK(batch_query_impl(e, g->qids.data(), n, nullptr, g->qdev(), (uint32_t)g->dim, g->dist.data(), g->rowp.data(),
                         g->okv.data()));
    uint64_t* rec = G.slow_h.as<uint64_t>() + (uint64_t)s * G.npos * G.W;
    for (uint64_t i = 0; i < n; ++i) {
      uint64_t* r = rec + i * G.W;
      const bool own = e->parts[g->qids[i] / e->PS].owned;
      for (uint32_t w = 0; w + 1 < G.W; ++w) r[w] = own && g->okv[i] ? g->rowp[i][G.w0 + w] : 0;
      uint32_t db;
      memcpy(&db, &g->dist[i], 4);
      r[G.W - 1] = own && g->okv[i] ? (1ull << 32) | db : 0;
    }
  }
  uint64_t* ids = G.ids_h.as<uint64_t>() + (uint64_t)s * G.npos;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t id = g->qids[i], p = id / e->PS;
    int32_t v = -1;
    if (e->parts[p].owned) {
      if (*fast)
        if (const uint32_t* j = e->resp_map.find(id)) v = (int32_t)*j;
    } else if (G.comb->model_peers) {   // answered by its partition's holder unless dropped (batch-pir.go:195-200)
      for (uint64_t j = 0; j < e->qn && j < e->pq[p].size(); ++j)
        if (e->pq[p][j] == id) { v = -2; break; }
    }
    map[i] = v;
    ids[i] = id;
  }
  G.slow[s] = !*fast;
  e->ctx->host_add(HT_BATCH_QUERY, ms_since(t));
  return 0;
}

// After the shared step (group_step): the records of this rank's answers, the
// multi-step sessions' host-packed records, the modelled peers' records, the
// combine, and one copy of all records (and the step's statuses) to the host.
//
// Failure protocol (every rank must issue the same collectives): the team's
// records end in ONE error word, 0 from a healthy rank.  A rank whose team (or
// another team of the same rank: ShardComb::abort) failed still takes the
// team's next combine turn, with zero records and the error word 1 (poison);
// every rank then reads a nonzero sum in that turn's records and stops the
// team there (group_collect_sharded).  So all ranks issue each team's
// collectives up to the same turn and none is left waiting in a collective.
static int group_exchange(StepGroup& G, const std::vector<char>& in, bool poison) {
  pm_ctx* c = G.c;
  hipStream_t st = c->stream;
  const uint32_t nrec = G.S * G.npos;
  const uint64_t nw = (uint64_t)nrec * G.W;
  uint32_t* st2 = G.st_d.as<uint32_t>();
  uint32_t nsub = poison ? 0u : G.nsub;
  // this rank's records (map, pack, multi-step sessions, modelled peers)
  auto pack = [&]() -> int {
    int32_t* map = G.map_h.as<int32_t>();
    for (uint32_t s = 0; s < G.S; ++s)   // client-local sub-query indices -> the shared step's
      for (uint32_t i = 0; i < G.npos; ++i) {
        int32_t& v = map[(uint64_t)s * G.npos + i];
        if (poison) v = -1;
        else if (v >= 0) v = in[s] ? v + (int32_t)G.base[s] : -1;
      }
    HIPCHK(hipMemcpyAsync(G.map_d.p, map, (uint64_t)nrec * 4, hipMemcpyHostToDevice, st));
    const PmOutHdr* hdr = G.out_d.as<PmOutHdr>();
    const uint64_t* rows = (const uint64_t*)(G.out_d.as<char>() + (uint64_t)G.nsub * sizeof(PmOutHdr));
    c->timed("pack_records", (double)nw * 8, [&] {
      pmk::pack_records(st, G.map_d.as<int32_t>(), nrec, hdr, rows, G.E, G.w0, G.W, G.rec_d, nsub, st2,
                        poison ? 1u : 0u); });
    for (uint32_t s = 0; s < G.S && !poison; ++s)
      if (G.slow[s])
        HIPCHK(hipMemcpyAsync(G.rec_d + (uint64_t)s * G.npos * G.W, G.slow_h.as<uint64_t>() + (uint64_t)s * G.npos * G.W,
                              (uint64_t)G.npos * G.W * 8, hipMemcpyHostToDevice, st));
    if (G.comb->model_peers && !poison) {
      HIPCHK(hipMemcpyAsync(G.ids_d.p, G.ids_h.p, (uint64_t)nrec * 8, hipMemcpyHostToDevice, st));
      const pm_graph* g0 = G.gs[0];
      c->timed("synth_records", 0, [&] {
        pmk::synth_records(st, G.map_d.as<int32_t>(), G.ids_d.as<uint64_t>(), nrec, G.npos, G.qbuf.as<float>(), G.dim,
                           (uint32_t)g0->m, g0->n, g0->data_seed, G.w0, G.W, G.rec_d); });
    }
    HIPCHK(hipGetLastError());
    return 0;
  };
  const int pre = pack();
  std::string pre_msg;
  if (pre) {
    // a failure before the collective: the turn is still owed to the peers.
    // Take it poisoned (zero records, error word 1) if the device still
    // accepts work; otherwise no further turn can match the peers' (they are
    // then bounded by their own RCCL / torch.distributed timeout).
    pre_msg = pm_last_error();
    poison = true;
    nsub = 0;
    const uint64_t one = 1;
    if (!G.comb->fn || hipMemsetAsync(G.rec_d, 0, nw * 8, st) != hipSuccess ||
        hipMemcpyAsync(G.rec_d + nw, &one, 8, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      G.combine_dead = true;
      return fail(pre, pre_msg);
    }
  }
  if (G.comb->fn) {   // the collective, in the global (round, team) order on every rank
    ShardComb* cb = G.comb;
    const uint64_t turn = G.round * cb->NG + G.team;
    auto tw = Clock::now();
    // no early exit on cb->abort: a failed team still takes its turn (poisoned);
    // bounded so a rank whose peer died ends instead of spinning forever
    static const double limit_s = [] { const char* e = getenv("PM_COMBINE_TIMEOUT_S"); return e ? atof(e) : 600.0; }();
    uint32_t spins = 0;
    while (cb->ticket.load(std::memory_order_acquire) != turn) {
      if (++spins % 1024 == 0 && ms_since(tw) > limit_s * 1e3) {
        G.combine_dead = true;
        return fail(PM_EHIP, "sharded search: combine turn " + std::to_string(turn) + " not reached in " +
                                 std::to_string(limit_s) + " s");
      }
      std::this_thread::yield();
    }
    c->host_add(HT_COMBINE_TURN, ms_since(tw));
    auto t0 = Clock::now();
    int rc = 0;
    c->timed("combine", (double)nw * 8, [&] { rc = cb->fn(cb->user, G.team, G.rec_d, nw + 1, (void*)st); });
    c->host_add(HT_COMBINE, ms_since(t0));
    cb->ticket.fetch_add(1, std::memory_order_acq_rel);
    G.round++;
    if (rc) {   // the collective itself failed: no further turn of this team can match the peers'
      G.combine_dead = true;
      return fail(PM_EHIP, "sharded search: the combine callback failed (" + std::to_string(rc) + ")");
    }
    if (pre) { G.peer_failed.store(true); return fail(pre, pre_msg); }   // the turn taken poisoned; this team stops
  } else {
    G.round++;
  }
  HIPCHK(hipMemcpyAsync(G.rec_h.p, G.rec_d, (nw + 1) * 8, hipMemcpyDeviceToHost, st));
  if (nsub) HIPCHK(hipMemcpyAsync(G.rec_h.as<uint64_t>() + nw + 1, st2, (uint64_t)nsub * 8, hipMemcpyDeviceToHost, st));
  G.seq = c->record_done(st);
  return 0;
}

// L2Dist in the reference's order (l2_distance_amd64.s:4-36 via
// build_graph.go:119-127): eight lane sums of separately rounded sub / mul /
// add, ((l0+l1)+(l2+l3))+((l4+l5)+(l6+l7)), then the scalar tail.  Host-side
// check of the GPU's records only (the translation unit is built without FMA
// contraction).
static float l2_reference_order(const float* a, const float* b, uint64_t dim) {
  const uint64_t dimS = dim & ~7ull;
  float l[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint64_t t = 0; t < dimS; t += 8)
    for (int k = 0; k < 8; ++k) {
      const float d = a[t + k] - b[t + k];
      const float sq = d * d;
      l[k] = l[k] + sq;
    }
  float d = dimS ? ((l[0] + l[1]) + (l[2] + l[3])) + ((l[4] + l[5]) + (l[6] + l[7])) : 0.0f;
  for (uint64_t i = dimS; i < dim; ++i) {
    const float x = a[i] - b[i];
    const float sq = x * x;
    d = d + sq;
  }
  return d;
}

// The record check (pm_set_option "verify_records"): every answered record of
// session s's batch against the graph itself (the synthetic spec or the host
// arrays) — neighbour words bit for bit, and the distance bits against
// l2_reference_order of the vertex's vector and the session's query — and
// every unanswered id against its explanation (private-search.go:441-506 over
// batch-pir.go:170-248).  Counts go to the session's host counters.
static void verify_records(StepGroup& G, uint32_t s, bool fast, const uint64_t* rec, const uint32_t* st2) {
  pm_graph* g = G.gs[s];
  Engine* e = G.es[s];
  const uint64_t dim = g->dim, m = g->m;
  const float* q = G.qstage.as<float>() + (uint64_t)s * dim;
  const uint64_t kv = sm64(g->data_seed + DOM_SYNTH_VEC);
  std::vector<float> vec(dim);
  uint32_t tmp[64];
  for (uint64_t i = 0; i < G.npos; ++i) {
    const uint64_t* r = rec + ((uint64_t)s * G.npos + i) * G.W;
    const uint64_t id = (uint64_t)g->batch[i], p = id / e->PS;
    const bool ok = (r[G.W - 1] >> 32) & 1;
    if (ok) {
      const uint32_t* nb = g->true_nb(id, tmp);
      if (g->synth) for (uint64_t j = 0; j < dim; ++j) vec[j] = graph_synth_vec(kv, id, (uint32_t)dim, (uint32_t)j);
      else memcpy(vec.data(), g->vectors + id * dim, dim * 4);
      const float d = l2_reference_order(vec.data(), q, dim);
      uint32_t dbits;
      memcpy(&dbits, &d, 4);
      const bool good = memcmp((const char*)r + G.nb_off, nb, m * 4) == 0 && (uint32_t)r[G.W - 1] == dbits;
      g->ctx->host_add(good ? HT_REC_VERIFIED : HT_REC_BAD, 0.0);
      continue;
    }
    bool made = false;   // was a sub-query made for it (among the first qn of its partition, batch-pir.go:195-200)?
    for (uint64_t j = 0; j < e->qn && j < e->pq[p].size(); ++j) made |= e->pq[p][j] == id;
    HostTimer why = HT_REC_UNEXPLAINED;
    if (!made) {
      why = HT_REC_DROPPED;
    } else if (!e->parts[p].owned) {
      why = G.comb->model_peers ? HT_REC_UNEXPLAINED : HT_REC_PEER;   // a modelled peer always answers
    } else if (!fast) {
      why = HT_REC_FAILED;   // the multi-step path: its sub-queries' statuses stay on the host path
    } else if (const uint32_t* j = e->resp_map.find(id)) {
      const uint32_t st = st2[2 * ((uint64_t)G.base[s] + *j)];
      if (st == ST_ENOHIT || st == ST_ECHUNK || st == ST_EBUDGET) why = HT_REC_FAILED;
    }
    g->ctx->host_add(why, 0.0);
  }
}

// Session s's share of the exchanged records: host mirrors of its sub-queries
// on this rank (post_results), the batch's counters and trigger (bq_tail), and
// the neighbour lists and distances of all its ids (Entry2VectorAndNeighbors,
// private-search.go:418-439, with the success check :483-497).
static int group_collect_sharded(StepGroup& G, uint32_t s, bool fast) {
  pm_graph* g = G.gs[s];
  Engine* e = G.es[s];
  auto t_wait = Clock::now();
  if (G.c->publish_wait) CHK(wait_done(G.c, G.seq));
  else HIPCHK(hipStreamSynchronize(G.c->stream));
  e->ctx->host_add(HT_STEP_WAIT, ms_since(t_wait));
  const uint64_t nw = (uint64_t)G.S * G.npos * G.W, m = g->m;
  const uint64_t* rec = G.rec_h.as<uint64_t>();
  if (rec[nw]) {   // the error word: rec[nw] ranks poisoned this turn (group_exchange)
    G.peer_failed.store(true);
    return fail(PM_EHIP, "sharded search: " + std::to_string(rec[nw]) + " rank(s) failed; this team stops at the "
                         "same combine turn on every rank");
  }
  const uint32_t* st2 = (const uint32_t*)(rec + nw + 1);
  if (fast) {
    auto tp = Clock::now();
    for (size_t j = 0; j < e->subs.size(); ++j) {
      const uint64_t k = G.base[s] + j;
      if (st2[2 * k] == ST_OK) {
        PartHost& ph = e->parts[e->subs[j].part];
        ph.fqn++;
        ph.cache.put(e->subs[j].idx, st2[2 * k + 1]);
      }
    }
    e->ctx->host_add(HT_STEP_POST, ms_since(tp));
    CHK(bq_tail(e, G.npos));
  }
  auto t_parse = Clock::now();
  uint32_t tmp[64];
  for (uint64_t i = 0; i < G.npos; ++i) {
    const uint64_t* r = rec + ((uint64_t)s * G.npos + i) * G.W;
    uint32_t* nbi = &g->nb[i * m];
    memcpy(nbi, (const char*)r + G.nb_off, m * 4);
    const uint32_t db = (uint32_t)r[G.W - 1];
    memcpy(&g->dist[i], &db, 4);
    if (memcmp(nbi, g->true_nb((uint64_t)g->batch[i], tmp), m * 4) == 0) g->succ++;
  }
  if (G.verify_every && (G.round - 1) % G.verify_every == 0) verify_records(G, s, fast, rec, st2);
  e->rows_partial = false;
  g->ctx->host_add(HT_GVI_PARSE, ms_since(t_parse));
  return 0;
}

// Buffers of a sharded team (after group_init).
static int group_shard_init(StepGroup& G, pm_graph** gs, uint32_t S, int parallel, ShardComb* comb, uint32_t team) {
  G.comb = comb;
  G.team = team;
  G.round = 0;
  G.verify_every = (uint32_t)g_verify_records.load();
  G.gs.assign(gs, gs + S);
  const Engine& e = gs[0]->pir->e;
  G.npos = (uint32_t)(parallel * gs[0]->m);
  G.w0 = (uint32_t)(gs[0]->dim * 4 / 8);
  const uint32_t w1 = (uint32_t)((gs[0]->dim * 4 + gs[0]->m * 4 + 7) / 8);
  G.W = w1 - G.w0 + 1;
  G.nb_off = (uint32_t)(gs[0]->dim * 4 - (uint64_t)G.w0 * 8);
  if (e.pf_off != (size_t)gs[0]->dim * 4) return fail(PM_EINVAL, "sharded search: entries are not PIRGraphInfo's");
  const uint64_t nrec = (uint64_t)S * G.npos, nw = nrec * G.W;
  if (comb->bufs) {
    G.rec_d = comb->bufs[team];
    if (!G.rec_d) return fail(PM_EINVAL, "sharded search: NULL team buffer");
  } else {
    CHK(G.rec_own.reserve((nw + 1) * 8));
    G.rec_d = G.rec_own.as<uint64_t>();
  }
  CHK(G.st_d.reserve(std::max<uint64_t>(8, nrec * 8)));   // at most one sub-query per position
  CHK(G.map_d.reserve(nrec * 4));
  CHK(G.ids_d.reserve(nrec * 8));
  CHK(G.map_h.reserve(nrec * 4));
  CHK(G.ids_h.reserve(nrec * 8));
  CHK(G.slow_h.reserve(nw * 8));
  CHK(G.rec_h.reserve((nw + 1) * 8 + nrec * 8));
  G.slow.assign(S, 0);
  if (!gs[0]->dvec->p) {   // the sessions' start vectors side by side for the team's one k_l2_rows launch
    const uint64_t per = (uint64_t)G.ns * G.dim;
    CHK(G.start_vec.reserve(std::max<uint64_t>(4, S * per * 4)));
    for (uint32_t i = 0; i < S; ++i)
      if (per) HIPCHK(hipMemcpyAsync(G.start_vec.as<float>() + i * per, gs[i]->dstartvec.p, per * 4,
                                     hipMemcpyDeviceToDevice, G.c->stream));
    HIPCHK(hipStreamSynchronize(G.c->stream));
  }
  return 0;
}

// A lock-step team's device setup over sessions gs[0..S) (gs[0]'s stream):
// start ids, query slots (each session's query pointer points into G.qbuf
// until team_release), the clients' parts.
static int team_init(StepGroup& G, pm_graph** gs, uint32_t S) {
  G.dim = (uint32_t)gs[0]->dim;
  G.rows_partial = true;   // GetVertexInfo reads the neighbour lists only
  for (uint32_t i = 0; i < S; ++i) G.es.push_back(&gs[i]->pir->e);
  HIPCHK(hipSetDevice(gs[0]->ctx->device));
  for (uint32_t i = 0; i < S; ++i) HIPCHK(hipStreamSynchronize(gs[i]->ctx->stream));
  G.ns = (uint32_t)gs[0]->start.size();
  for (uint32_t i = 0; i < S; ++i)
    if (gs[i]->start.size() != G.ns) return fail(PM_EINVAL, "sessions with different start-set sizes");
  CHK(G.qbuf.reserve((uint64_t)S * G.dim * 4));
  CHK(G.start_ids.reserve(std::max<uint64_t>(4, (uint64_t)S * G.ns * 4)));
  CHK(G.start_dist.reserve(std::max<uint64_t>(4, (uint64_t)S * G.ns * 4)));
  CHK(G.qstage.reserve((uint64_t)S * (G.dim + G.ns) * 4));
  {
    std::vector<uint32_t> ids;
    for (uint32_t i = 0; i < S; ++i) ids.insert(ids.end(), gs[i]->start.begin(), gs[i]->start.end());
    if (!ids.empty()) HIPCHK(hipMemcpy(G.start_ids.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice));
  }
  for (uint32_t i = 0; i < S; ++i) {
    gs[i]->q_shared = G.qbuf.as<float>() + (uint64_t)i * G.dim;
    G.qv.push_back(gs[i]->qdev());
  }
  return group_init(G, gs[0]->ctx);
}
static void team_release(pm_graph** gs, uint32_t S) {
  for (uint32_t i = 0; i < S; ++i) gs[i]->q_shared = nullptr;
}

// One lock-step team: sessions gs[0..S) share one step stream (gs[0]'s) and T
// worker threads; maintenance seconds into mt[0..S).  Runs on the calling thread.
static int run_batched_team(pm_graph** gs, uint32_t S, const float* queries, uint64_t q, int k, int step,
                            int parallel, uint32_t T, int64_t* answers, double* mt_out, ShardComb* comb = nullptr,
                            uint32_t team = 0) {
  StepGroup G;
  struct Unshare {   // the sessions' query pointers point into G.qbuf until the team ends
    pm_graph** gs; uint32_t S;
    ~Unshare() { team_release(gs, S); }
  } unshare{gs, S};
  CHK(team_init(G, gs, S));
  if (comb) CHK(group_shard_init(G, gs, S, parallel, comb, team));
  T = std::max(1u, std::min(T, S));
  std::vector<char> fast(S, 0), need_prep(S, 0);
  std::vector<double> mt(S, 0.0);
  std::atomic<int> err{0};
  std::string err_msg;
  std::atomic<bool> stop{false};
  SpinBarrier bar;
  bar.n = T;
  auto set_err = [&](int rc, uint32_t s) {
    int z = 0;
    if (rc && err.compare_exchange_strong(z, rc)) err_msg = "session " + std::to_string(s) + ": " + pm_last_error();
    if (rc && comb) comb->abort.store(true);   // the other teams stop waiting for this one's turns
  };
  std::vector<int64_t> steps_buf((size_t)T * std::max(k, 1));
  // worker w serves sessions s = w, w + T, ...; worker 0 (this thread) also launches the shared steps
  auto worker = [&](uint32_t w) {
    if (hipSetDevice(G.c->device) != hipSuccess) set_err(PM_EHIP, w);
    int64_t* stp = &steps_buf[(size_t)w * std::max(k, 1)];
    for (uint64_t qi = 0; qi < q; ++qi) {
      // SearchKNN begin: every session's query and start-set distances in one
      // upload, one k_l2_rows launch and one download for the team
      float* qst = G.qstage.as<float>();
      for (uint32_t s = w; s < S; s += T) {
        pm_graph* g = gs[s];
        knn_reset(g);
        g->t_init = Clock::now();
        memcpy(qst + (uint64_t)s * G.dim, queries + ((uint64_t)s * q + qi) * g->dim, G.dim * 4);
      }
      bar.wait();
      if (w == 0 && !err.load()) {
        const int rc = group_start_dist(G, gs);
        if (rc) set_err(rc, 0);
      }
      bar.wait();
      for (uint32_t s = w; s < S && !err.load(); s += T)
        knn_begin_finish(gs[s], parallel, 0, qst + (uint64_t)S * G.dim + (uint64_t)s * G.ns);
      for (int st = 0; st < step; ++st) {
        for (uint32_t s = w; s < S && !err.load(); s += T) {   // this round's ids -> sub-queries
          pm_graph* g = gs[s];
          knn_batch(g, parallel, 0);
          bool f = false;
          const int rc = comb ? gvi_pre_sharded(g, G, s, &f) : gvi_pre(g, true, &f);
          fast[s] = f;
          if (rc) set_err(rc, s);
        }
        bar.wait();
        if (w == 0) {
          if (comb && comb->fn) {   // sharded: this round's combine is taken on every rank (see group_exchange)
            if (G.peer_failed.load() || G.combine_dead) {
              stop.store(true);
            } else {
              bool poison = err.load() != 0 || comb->abort.load();
              // fault seam (tests/test_shard_search_gpu.py): team 0 fails at shared step PM_FAULT_ROUND
              static const long fault_round = [] { const char* e = getenv("PM_FAULT_ROUND"); return e ? atol(e) : -1L; }();
              if (!poison && team == 0 && fault_round >= 0 && G.round == (uint64_t)fault_round) {
                set_err(fail(PM_EHIP, "injected fault (PM_FAULT_ROUND)"), 0);
                poison = true;
              }
              if (!poison) {
                const int rc = group_step(G, fast);
                if (rc) set_err(rc, 0);
                poison = rc != 0;
              }
              const int rx = group_exchange(G, fast, poison);   // records, combine, read-back
              if (rx) set_err(rx, 0);
              stop.store(poison || rx != 0);
            }
          } else {
            if (!err.load()) {
              int rc = group_step(G, fast);
              if (!rc && comb) rc = group_exchange(G, fast, false);   // records, read-back (no collective)
              if (rc) set_err(rc, 0);
            }
            stop.store(err.load() != 0);
          }
        }
        bar.wait();
        if (stop.load()) return;
        for (uint32_t s = w; s < S && !err.load(); s += T) {   // rows -> neighbours, known set
          pm_graph* g = gs[s];
          if (comb) {   // every id's record, combined over the shards
            const int rw = group_collect_sharded(G, s, fast[s]);
            if (rw) { set_err(rw, s); break; }
          } else {
            if (fast[s]) {   // this client's share of the shared step's results
              const int rw = group_collect(G, s);
              if (rw) { set_err(rw, s); break; }
            }
            const int rc = gvi_post(g, true, fast[s]);
            if (rc) { set_err(rc, s); break; }
          }
          knn_update(g, st);
        }
      }
      for (uint32_t s = w; s < S && !err.load(); s += T) {   // top k, maintenance trigger (private-search.go:226-232)
        pm_graph* g = gs[s];
        knn_end(g, k, answers + ((uint64_t)s * q + qi) * k, stp);
        Engine* e = &g->pir->e;
        need_prep[s] = e->FBN + (uint64_t)step * (uint64_t)parallel + 10 >= e->Support;
      }
      bar.wait();
      if (w == 0) {   // the triggered clients' preprocessings as one launch set
        if (!err.load()) {
          const int rc = group_prep(G, need_prep, &mt);
          if (rc) set_err(rc, 0);
        }
        stop.store(err.load() != 0);
        // a sharded team that failed here still owes its peers its next combine turn, poisoned
        if (stop.load() && comb && comb->fn && !G.peer_failed.load() && !G.combine_dead && qi + 1 < q)
          (void)group_exchange(G, fast, true);
      }
      bar.wait();
      if (stop.load()) return;
    }
  };
  std::vector<std::thread> th;
  for (uint32_t w = 1; w < T; ++w) th.emplace_back(worker, w);
  worker(0);
  for (auto& t : th) t.join();
  if (err.load()) return fail(err.load(), err_msg);
  HIPCHK(hipStreamSynchronize(G.c->stream));
  for (uint32_t s = 0; s < S; ++s) mt_out[s] = mt[s];
  return 0;
}

// ---- SimpleBatchPianoPIR clients served together (the batch API) --------
// S clients of one server (pm_batchpir_create_client): every call answers one
// batch of n ids per client (SimpleBatchPianoPIR.Query, batch-pir.go:170-248,
// per client) with ONE shared step over all their partitions.
struct pm_batchpir_group {
  StepGroup G;
  std::vector<char> fast;
};
extern "C" int pm_batchpir_group_create(pm_batchpir** clients, uint32_t S, pm_batchpir_group** out) {
  if (!clients || !S || !out) return fail(PM_EINVAL, "NULL argument");
  for (uint32_t i = 0; i < S; ++i) {
    if (!clients[i]) return fail(PM_EINVAL, "NULL client");
    const Engine& a = clients[0]->e;
    const Engine& b = clients[i]->e;
    if (a.db.get() != b.db.get() || a.P != b.P || a.E != b.E || a.N != b.N || a.shard != b.shard ||
        a.nshards != b.nshards || b.ctx->device != a.ctx->device || !b.is_batch)
      return fail(PM_EINVAL, "grouped clients must be batch PIR clients of one server on one device");
    for (uint32_t j = 0; j < i; ++j)
      if (clients[j] == clients[i]) return fail(PM_EINVAL, "a client appears twice");
  }
  pm_batchpir_group* h = new pm_batchpir_group();
  for (uint32_t i = 0; i < S; ++i) h->G.es.push_back(&clients[i]->e);
  h->fast.assign(S, 0);
  for (uint32_t i = 0; i < S; ++i) {
    const hipError_t e = hipStreamSynchronize(clients[i]->e.ctx->stream);
    if (e != hipSuccess) { delete h; return fail(PM_EHIP, hipGetErrorString(e)); }
  }
  if (int r = group_init(h->G, clients[0]->e.ctx)) { delete h; return r; }
  *out = h;
  return 0;
}
extern "C" void pm_batchpir_group_destroy(pm_batchpir_group* h) { delete h; }
extern "C" int pm_batchpir_group_preprocessing(pm_batchpir_group* h) {
  if (!h) return fail(PM_EINVAL, "NULL argument");
  // SimpleBatchPianoPIR.Preprocessing (batch-pir.go:119-155) of every client,
  // as ONE launch set: each partition's K clients fold side by side
  return group_prep(h->G, std::vector<char>(h->G.S, 1), nullptr);
}
extern "C" int pm_batchpir_group_query(pm_batchpir_group* h, const uint64_t* ids, uint64_t n, uint64_t* out,
                                       uint8_t* ok) {
  if (!h || (!ids && n) || (!out && n)) return fail(PM_EINVAL, "NULL argument");
  StepGroup& G = h->G;
  const uint64_t E = G.E;
  for (uint32_t s = 0; s < G.S; ++s) {   // bucketing; clients at a partition's budget go alone
    Engine* e = G.es[s];
    bool f = false;
    CHK(bq_prepare(e, ids + (uint64_t)s * n, n, &f));
    h->fast[s] = f;
    if (!f)
      CHK(batch_query_impl(e, ids + (uint64_t)s * n, n, out + (uint64_t)s * n * E, nullptr, 0, nullptr, nullptr,
                           ok ? ok + (uint64_t)s * n : nullptr));
  }
  CHK(group_step(G, h->fast));
  for (uint32_t s = 0; s < G.S; ++s) {
    if (!h->fast[s]) continue;
    Engine* e = G.es[s];
    CHK(group_collect(G, s));
    bq_emit_fast(e, ids + (uint64_t)s * n, n, out + (uint64_t)s * n * E, nullptr, nullptr,
                 ok ? ok + (uint64_t)s * n : nullptr);
    CHK(bq_tail(e, n));
  }
  return 0;
}

// pm_search_loop_batched with the host work pooled (the default; PM_BATCH_POOL=0:
// one worker subset per team, run_batched_team).  The NG lock-step teams keep
// their shared steps (one stream each, the same launches), but every worker
// serves every team: when a team's step has completed, all workers take its
// sessions' host work (results, GetVertexInfo's post-processing, the search
// update, the next round's ids and bucketing), one session at a time off an
// atomic counter, and the worker that finishes the team's last session
// launches its next step -- or, at the end of a query, runs its maintenance
// and the next query's start (search.go:130-146).  A team's host phase then
// takes about 1/T of its sessions' host time instead of NG/T, so the GPU is not
// left waiting while a fixed subset of workers works through one team, and
// teams that fall behind get more of the workers.  Every session performs the
// same operations in the same order as in run_batched_team.
// PM_TEAM_TRACE=<file> (diagnostics): the pooled loop's host spans, one CSV row
// each: team, kind (0 session task, 1 step launch, 2 maintenance, 3 query
// start, 4 step in flight until seen complete), worker, start and end in us.
// Host trace of the pooled loop (PM_TEAM_TRACE=<file>): one record per task,
// launch, maintenance, query start and step flight, kept per worker (no lock
// on the serving path) and written when the loop ends.
struct TeamTrace {
  struct Rec { double t0, t1; uint32_t team, kind, worker; };
  const char* file = getenv("PM_TEAM_TRACE");
  Clock::time_point base = Clock::now();
  std::vector<std::vector<Rec>> recs;   // [worker]
  explicit TeamTrace(uint32_t workers) { if (file) { recs.resize(workers); for (auto& v : recs) v.reserve(1 << 16); } }
  double now() const { return std::chrono::duration<double, std::micro>(Clock::now() - base).count(); }
  static inline thread_local uint32_t tl_worker = 0;   // the calling worker (set when it starts)
  void add(double t0, uint32_t team, uint32_t kind, uint32_t /*worker*/) {
    if (!file) return;
    recs[tl_worker].push_back({t0, now(), team, kind, tl_worker});
  }
  ~TeamTrace() {
    if (!file) return;
    if (FILE* f = fopen(file, "w")) {
      fprintf(f, "team,kind,worker,t0_us,t1_us\n");
      for (auto& v : recs)
        for (auto& r : v) fprintf(f, "%u,%u,%u,%.2f,%.2f\n", r.team, r.kind, r.worker, r.t0, r.t1);
      fclose(f);
    }
  }
};
enum : int { kTeamStart, kTeamOpen, kTeamBusy, kTeamFlight, kTeamPrep, kTeamDone };
constexpr uint32_t kNoSession = ~0u;
struct PoolTeam {
  StepGroup G;
  pm_graph** gs = nullptr;
  uint32_t S = 0, s0 = 0;
  std::vector<char> fast, need_prep;
  std::vector<double> mt;
  std::atomic<uint64_t> qi{0};     // the team's current query (read by the merged maintenance's worker)
  int st = 0;                      // its current round
  bool begin = false;              // the open phase: a query's start (true) or a round's results
  std::atomic<int> state{kTeamStart};
  std::unique_ptr<std::atomic<uint32_t>[]> lane;   // per worker w: sessions w, w + T, ... taken so far
  std::atomic<uint32_t> ndone{0};
  Clock::time_point launched, prep_since;
  double launched_us = 0;
  uint32_t id = 0;
};
// Streams of the lock-step teams.  A team's steps ran on its first session's
// context stream, and every session context creates its stream when it is
// made: HIP maps streams onto the process's GPU_MAX_HW_QUEUES (4) hardware
// queues in creation order, so with 72 sessions per team the four teams'
// streams (sessions 0, 72, 144, 216) could all land on ONE hardware queue,
// whose in-order packets serialise the teams' kernels.  The teams get streams
// of their own instead, created back to back once per device (so they take
// distinct hardware queues), swapped into the team's context for the loop
// (the context streams where none can be created).
static hipStream_t team_stream(int dev, uint32_t t) {
  static std::mutex mu;
  static std::vector<hipStream_t> pool[64];
  if (dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  std::vector<hipStream_t>& v = pool[dev];
  if (v.empty()) {
    for (int i = 0; i < 8; ++i) {
      hipStream_t st = nullptr;
      if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) st = nullptr;
      if (!st) break;
      v.push_back(st);
    }
  }
  return v.empty() ? nullptr : v[t % v.size()];
}
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

static int run_batched_pool(pm_graph** gs, uint32_t S, const float* queries, uint64_t q, int k, int step, int parallel,
                            uint32_t NG, uint32_t T, int64_t* answers, double* mt_out) {
  std::vector<StreamSwap> swaps(NG);   // destroyed after `teams` (declared first): streams drained, restored
  std::vector<std::unique_ptr<PoolTeam>> teams;
  DevBuf prep_buf;   // the merged maintenance's parts
  std::mutex prep_mu;
  // Maintenance (the end-of-query re-preprocessing, private-search.go:226-232)
  // of the teams that need it at the same query runs as ONE launch set: a team
  // whose clients need it after query Q waits (kTeamPrep) until every other
  // team has finished query Q (it waits at Q too, has moved past Q, or is
  // done); the teams waiting at Q are then re-preprocessed together.  The set
  // is a function of the sessions' triggers alone (no timeout: the bench's
  // 256 sessions always fold in one launch, which the headline parity test
  // asserts), and no wait is unbounded: every other team is running its query
  // Q.  The maintenance kernels fill the GPU, so teams' maintenances run one
  // after another either way; merged, the teams also resume together instead
  // of finishing the timed work one after another with the GPU partly idle.
  struct Release {
    std::vector<std::unique_ptr<PoolTeam>>& t;
    ~Release() { for (auto& x : t) team_release(x->gs, x->S); }
  } release{teams};
  for (uint32_t g = 0; g < NG; ++g) {
    const uint32_t s0 = (uint32_t)((uint64_t)S * g / NG), s1 = (uint32_t)((uint64_t)S * (g + 1) / NG);
    teams.emplace_back(new PoolTeam());
    PoolTeam& t = *teams.back();
    t.gs = gs + s0; t.S = s1 - s0; t.s0 = s0; t.id = g;
    t.fast.assign(t.S, 0); t.need_prep.assign(t.S, 0); t.mt.assign(t.S, 0.0);
    t.lane.reset(new std::atomic<uint32_t>[T]);
    for (uint32_t w = 0; w < T; ++w) t.lane[w].store(0);
    CHK(team_init(t.G, t.gs, t.S));
    swaps[g].swap_in(t.G.c, team_stream(t.G.c->device, g));
    static const int stage = [] { const char* e = getenv("PM_DESC_STAGE"); return e ? atoi(e) : 1; }();
    t.G.stage_on = stage != 0;
    t.G.stg.resize(t.S);
  }
  const uint32_t dim = (uint32_t)gs[0]->dim;
  TeamTrace tr(T);
  std::atomic<int> err{0};
  std::atomic<uint32_t> finished{0};
  std::string err_msg;
  std::mutex err_mu;
  auto set_err = [&](int rc, uint32_t s) {
    std::lock_guard<std::mutex> lk(err_mu);
    int z = 0;
    if (rc && err.compare_exchange_strong(z, rc)) err_msg = "session " + std::to_string(s) + ": " + pm_last_error();
  };
  // the team's phase opens: its sessions' tasks become available
  auto open = [&](PoolTeam& t, bool begin) {
    t.begin = begin;
    t.ndone.store(0, std::memory_order_relaxed);
    for (uint32_t w = 0; w < T; ++w) t.lane[w].store(0, std::memory_order_release);
    t.state.store(kTeamOpen, std::memory_order_release);
  };
  // a session of the open phase: worker w's own lane first (sessions i = w mod
  // T: the same worker, hence core, serves a session every round and finds its
  // search state and prefetched rows in cache), then the other lanes' leftovers
  auto claim = [&](PoolTeam& t, uint32_t w) -> uint32_t {
    for (uint32_t j = 0; j < T; ++j) {
      const uint32_t l = (w + j) % T;
      if (l >= t.S) continue;
      if (t.lane[l].load(std::memory_order_relaxed) * T + l >= t.S) continue;
      const uint32_t i = t.lane[l].fetch_add(1, std::memory_order_acq_rel) * T + l;
      if (i < t.S) return i;
    }
    return kNoSession;
  };
  // SearchKNN begin for every session of the team: queries and start-set
  // distances in one upload, one k_l2_rows launch and one download
  auto start_query = [&](PoolTeam& t) -> int {
    const double t0 = tr.now();
    float* qst = t.G.qstage.as<float>();
    for (uint32_t i = 0; i < t.S; ++i) {
      pm_graph* g = t.gs[i];
      knn_reset(g);
      g->t_init = Clock::now();
      memcpy(qst + (uint64_t)i * dim, queries + ((uint64_t)(t.s0 + i) * q + t.qi) * dim, (size_t)dim * 4);
    }
    CHK(group_start_dist(t.G, t.gs));
    tr.add(t0, t.id, 3, 0);
    open(t, true);
    return 0;
  };
  // one session's share of the open phase (run_batched_team's per-session work)
  auto task = [&](PoolTeam& t, uint32_t i, int64_t* stp) -> int {
    pm_graph* g = t.gs[i];
    if (t.begin) {
      knn_begin_finish(g, parallel, 0, t.G.qstage.as<float>() + (uint64_t)t.S * dim + (uint64_t)i * t.G.ns);
    } else {
      // the next session of this worker's lane, one task ahead (prefetch_session)
      if (i + T < t.S && t.fast[i + T] && !t.G.comb) prefetch_session(t.G, i + T, t.gs[i + T]);
      if (g->graph) {   // the ground-truth rows of the success check (gvi_post), requested before the results' reads
        const uint64_t m = g->m;
        for (size_t b = 0; b < g->batch.size(); ++b) {
          const char* gr = (const char*)&g->graph[(uint64_t)g->batch[b] * m];
          __builtin_prefetch(gr);
          __builtin_prefetch(gr + m * 4 - 1);
        }
      }
      if (t.fast[i]) CHK(group_collect(t.G, i));   // complete: only the tokens and host mirrors
      CHK(gvi_post(g, true, t.fast[i]));
      knn_update(g, t.st);
      if (t.st + 1 == step) {   // top k, maintenance trigger (private-search.go:226-232)
        knn_end(g, k, answers + ((uint64_t)(t.s0 + i) * q + t.qi) * k, stp);
        Engine* e = &g->pir->e;
        t.need_prep[i] = e->FBN + (uint64_t)step * (uint64_t)parallel + 10 >= e->Support;
        return 0;
      }
    }
    knn_batch(g, parallel, 0);   // the next round's ids -> sub-queries
    bool f = false;
    CHK(gvi_pre(g, true, &f));
    t.fast[i] = f;
    if (f) group_stage_session(t.G, i);
    return 0;
  };
  // the worker that completed the phase's last session moves the team on
  auto advance = [&](PoolTeam& t) -> int {
    if (t.begin || t.st + 1 < step) {   // a round's ids are bucketed: its shared step
      t.st = t.begin ? 0 : t.st + 1;
      const double t0 = tr.now();
      CHK(group_step(t.G, t.fast));
      tr.add(t0, t.id, 1, 0);
      t.launched = Clock::now();
      t.launched_us = tr.now();
      t.state.store(kTeamFlight, std::memory_order_release);
      return 0;
    }
    const double t0 = tr.now();
    bool any = false;
    for (char c : t.need_prep) any |= c != 0;
    if (any) {   // with the other teams' (above)
      t.prep_since = Clock::now();
      t.state.store(kTeamPrep, std::memory_order_release);
      return 0;
    }
    CHK(group_prep(t.G, t.need_prep, &t.mt));   // the triggered clients' preprocessings as one launch set
    tr.add(t0, t.id, 2, 0);
    if (++t.qi == q) {
      t.state.store(kTeamDone, std::memory_order_release);
      finished.fetch_add(1);
      return 0;
    }
    return start_query(t);
  };
  std::vector<int64_t> steps_buf((size_t)T * std::max(k, 1));
  const int dev = gs[0]->ctx->device;
  auto worker = [&](uint32_t w) {
    TeamTrace::tl_worker = w;
    if (hipSetDevice(dev) != hipSuccess) { set_err(PM_EHIP, 0); return; }
    int64_t* stp = &steps_buf[(size_t)w * std::max(k, 1)];
    uint32_t idle = 0;
    while (!err.load(std::memory_order_relaxed) && finished.load(std::memory_order_acquire) < NG) {
      bool did = false;
      for (uint32_t j = 0; j < NG && !did; ++j) {
        PoolTeam& t = *teams[(w + j) % NG];
        int cur = t.state.load(std::memory_order_acquire);
        if (cur == kTeamOpen) {
          const uint32_t i = claim(t, w);
          if (i == kNoSession) continue;
          did = true;
          const double t0 = tr.now();
          int rc = task(t, i, stp);
          tr.add(t0, t.id, 0, w);
          if (rc) set_err(rc, t.s0 + i);
          if (t.ndone.fetch_add(1, std::memory_order_acq_rel) + 1 == t.S && !err.load()) {
            t.state.store(kTeamBusy, std::memory_order_relaxed);
            rc = advance(t);
            if (rc) set_err(rc, t.s0);
          }
        } else if (cur == kTeamPrep) {
          if (!prep_mu.try_lock()) continue;   // one worker runs the merged maintenance
          std::lock_guard<std::mutex> lk(prep_mu, std::adopt_lock);
          // Q: the earliest query a team waits at; the set: the teams waiting at Q,
          // once every team still running has finished query Q
          uint64_t Q = ~0ull;
          for (auto& u : teams)
            if (u->state.load(std::memory_order_acquire) == kTeamPrep) Q = std::min(Q, u->qi.load(std::memory_order_acquire));
          if (Q == ~0ull) continue;
          bool all = true;
          for (auto& u : teams) {
            const int us = u->state.load(std::memory_order_acquire);
            if (us != kTeamPrep && us != kTeamDone && u->qi.load(std::memory_order_acquire) <= Q) all = false;
          }
          if (!all) continue;
          std::vector<PoolTeam*> ts;
          for (auto& u : teams) {
            int e = kTeamPrep;
            if (u->qi.load(std::memory_order_acquire) == Q &&
                u->state.compare_exchange_strong(e, kTeamBusy, std::memory_order_acq_rel))
              ts.push_back(u.get());
          }
          if (ts.empty()) continue;
          did = true;
          const double t0 = tr.now();
          std::vector<Engine*> who;
          std::vector<double*> mts;
          for (PoolTeam* u : ts)
            for (uint32_t s = 0; s < u->S; ++s)
              if (u->need_prep[s]) { who.push_back(u->G.es[s]); mts.push_back(&u->mt[s]); }
          const int rc = prep_clients(ts[0]->G.c, prep_buf, ts[0]->G.lp, who, &mts);
          if (rc) { set_err(rc, ts[0]->s0); break; }
          for (PoolTeam* u : ts) {
            tr.add(t0, u->id, 2, w);
            if (++u->qi == q) {
              u->state.store(kTeamDone, std::memory_order_release);
              finished.fetch_add(1);
            } else {
              u->state.store(kTeamStart, std::memory_order_release);   // a worker starts its next query
            }
          }
        } else if (cur == kTeamStart || cur == kTeamFlight) {
          bool ready = cur == kTeamStart;
          if (!ready) {
            const int rc = poll_done(t.G.c, t.G.seq, &ready);
            if (rc) { set_err(rc, t.s0); break; }
            if (!ready && std::chrono::duration<double>(Clock::now() - t.launched).count() > 10.0) {
              set_err(fail(PM_EHIP, "shared step not complete after 10 s"), t.s0);
              break;
            }
          }
          if (ready && t.state.compare_exchange_strong(cur, kTeamBusy, std::memory_order_acq_rel)) {
            did = true;
            if (cur == kTeamFlight) tr.add(t.launched_us, t.id, 4, w);
            const int rc = cur == kTeamStart ? start_query(t) : (open(t, false), 0);
            if (rc) set_err(rc, t.s0);
          }
        }
      }
      if (did) {
        idle = 0;
      } else if (++idle > 32) {   // nothing to do: give the core to the workers that have work
        std::this_thread::yield();
      } else {
        __builtin_ia32_pause();   // spin politely (an SMT sibling may be a working worker)
      }
    }
  };
  std::vector<std::thread> th;
  for (uint32_t w = 1; w < T; ++w) th.emplace_back(worker, w);
  worker(0);
  for (auto& t : th) t.join();
  for (auto& t : teams) HIPCHK(hipStreamSynchronize(t->G.c->stream));
  if (err.load()) return fail(err.load(), err_msg);
  for (auto& t : teams)
    for (uint32_t s = 0; s < t->S; ++s) mt_out[t->s0 + s] = t->mt[s];
  return 0;
}

// ---- the device loop (pm_drl.hip) -------------------------
// The batched serving loop with each team's rounds chained on the GPU: per
// query and team, [queries -> qbuf, start-set L2, k_team_round BEGIN], then per
// round [k_match_resolve_s, k_answer_p, k_team_round MID / END] on the team's
// stream, enqueued ahead; the host only decides the maintenance between
// queries (its schedule is a function of the counters alone) and runs it as
// one launch set of every triggered client, like run_batched_pool.  Taken when
// drl_plan shows that every round of the call would take the host's one-step
// path (no partition at its query budget, no batch-layer re-preprocessing);
// otherwise, or with pm_set_option("device_loop", 0) / PM_DEVICE_LOOP=0, the
// host loop serves the call.  Every session's answers, counters and state
// equal the host loop's (tests/test_gpu_parity.py, test_gpu_headline.py).
static bool device_loop_on() {
  const int o = g_device_loop.load();
  if (o >= 0) return o != 0;
  static const int env = [] { const char* e = getenv("PM_DEVICE_LOOP"); return e ? atoi(e) : 1; }();
  return env != 0;
}
static uint32_t pow2_at_least(uint64_t x) { uint32_t c = 1; while (c < x) c *= 2; return c; }

struct DrlShape { uint32_t n = 0, qn = 0, kcap = 0, cmask = 0; };
// Whether the device loop can serve the call, and its shape.  The counters
// FinishedBatchNum / QueriesMadeInPartition advance by fixed amounts per round
// (n / B, queryNumToMake) and reset at the harness's maintenance
// (private-search.go:226-232), so the whole call's schedule is known here: a
// query is chained on the device only if no round of it can reach a
// partition's budget (FinishedQueryNum + real sub-queries >= MaxQueryNum:
// bq_prepare's slow path; FinishedQueryNum <= QueriesMadeInPartition always)
// or the batch layer's trigger (QueriesMadeInPartition >= MaxQueryNum - 2).
static bool drl_plan(pm_graph** gs, uint32_t S, uint64_t q, int k, int step, int parallel, DrlShape* sh) {
  if (!device_loop_on() || S == 0 || step <= 0 || parallel <= 0 || k <= 0 || (uint32_t)parallel > pmk::kDrlMaxParallel)
    return false;
  const pm_graph* g0 = gs[0];
  const Engine& e0 = g0->pir->e;
  const uint64_t m = g0->m, n = (uint64_t)parallel * m, P = e0.P;
  if (m == 0 || m > 64 || n > pmk::kDrlMaxN || n * m > pmk::kDrlMaxNM || P == 0 || P > 64) return false;
  const uint64_t qn = n / P;
  if (qn == 0 || qn > pmk::step_max_sub_per_part() || e0.B == 0) return false;
  const uint64_t kcap = pow2_at_least((uint64_t)parallel + (uint64_t)step * n);
  if (kcap > pmk::kDrlMaxKcap || (uint64_t)k > kcap || pmk::team_round_lds(kcap, n, m) > 64 * 1024) return false;
  uint64_t maxq = ~0ull;
  for (uint32_t i = 0; i < S; ++i) {
    const pm_graph* g = gs[i];
    const Engine& e = g->pir->e;
    if (g->nonprivate || g->synth || !g->graph || !g->dvec->p || e.nshards != 1 || e.P != P || e.B != e0.B ||
        e.pf_off != g->dim * 4 || g->dim > 0xffffffffull || g->n >= 0xffffffffull || e.PS >= 0xffffffffull)
      return false;
    uint64_t mq = ~0ull;
    for (const PartHost& ph : e.parts) {
      mq = std::min(mq, ph.maxq64);
      maxq = std::max<uint64_t>(maxq == ~0ull ? 0 : maxq, ph.maxq64);   // localCache entries per partition <= MaxQueryNum
      if (ph.fqn > e.QMIP) return false;   // the bound below needs FinishedQueryNum <= QueriesMadeInPartition
    }
    uint64_t fbn = e.FBN, qmip = e.QMIP;
    for (uint64_t qi = 0; qi < q; ++qi) {
      if (qmip + (uint64_t)step * qn >= mq || qmip + (uint64_t)(step - 1) * qn + 2 >= e.parts[0].maxq64) return false;
      fbn += (uint64_t)step * (n / e.B);
      qmip += (uint64_t)step * qn;
      if (fbn + (uint64_t)step * (uint64_t)parallel + 10 >= e.Support) fbn = qmip = 0;
    }
  }
  sh->n = (uint32_t)n; sh->qn = (uint32_t)qn; sh->kcap = (uint32_t)kcap;
  sh->cmask = pow2_at_least(2 * std::max<uint64_t>(maxq, 1)) - 1;
  return true;
}

// The localCache indexes on the device for the loop: the device copy is made
// from the host's FlatMaps where it is not current (empty after a
// maintenance: a memset), and from then on the device copy is the truth.
static int ensure_dev_cache(Engine* e, uint32_t cmask, hipStream_t st) {
  const uint64_t cap = (uint64_t)cmask + 1, words = e->P * cap;
  if (e->dcache_cmask != cmask || !e->dcache.p) {
    if (e->cache_on_dev) CHK(ensure_host_cache(e));
    CHK(e->dcache.reserve(words * 8));
    e->dcache_cmask = cmask;
    e->dcache_valid = false;
  }
  if (!e->dcache_valid) {
    bool any = false;
    for (const PartHost& ph : e->parts) any |= ph.cache.count > 0;
    if (!any) {
      HIPCHK(hipMemsetAsync(e->dcache.p, 0, words * 8, st));
    } else {
      std::vector<uint64_t> t(words, 0);
      for (uint64_t p = 0; p < e->P; ++p)
        e->parts[p].cache.for_each([&](uint64_t key, uint32_t val) {
          uint64_t* tp = &t[p * cap];
          for (uint32_t i = pm::drl_hash((uint32_t)key) & cmask;; i = (i + 1) & cmask)
            if (!tp[i]) { tp[i] = ((uint64_t)val << 32) | (uint64_t)((uint32_t)key + 1u); break; }
        });
      HIPCHK(hipStreamSynchronize(st));
      HIPCHK(hipMemcpy(e->dcache.p, t.data(), words * 8, hipMemcpyHostToDevice));
    }
    e->dcache_valid = true;
  }
  e->cache_on_dev = true;
  return 0;
}

struct DrlTeam {
  StepGroup G;
  pm_graph** gs = nullptr;
  uint32_t S = 0, s0 = 0, nsub = 0;
  DevBuf sess, dummy, batch, heap, ktab, knb, kdist, kid, ctabp, answers, gid, out, allq, part_bytes, step_bytes,
      step_real, stamps;
  DrlArgs A{};
  hipEvent_t ev_end = nullptr;
  HostBuf prep_stage, parts_stage;               // pinned stages of the asynchronous maintenance (run_batched_dev)
  hipEvent_t prep_stage_ev = nullptr, parts_stage_ev = nullptr;
  DevBuf prep_buf;
  uint32_t seq = 0;                              // shared steps built so far (step_bytes rows)
  std::vector<std::pair<size_t, uint32_t>> tl;   // timed "answer" / "match_resolve" launches: (index, step)
  std::vector<char> need;
  std::vector<double> mt;
  ~DrlTeam() {
    for (hipEvent_t e : {ev_end, prep_stage_ev, parts_stage_ev})
      if (e) (void)hipEventDestroy(e);
  }
};

// The team's parts (new keys after a maintenance) up from a pinned stage on
// stream st, nothing waiting (the stage's previous copy is waited for first).
static int group_upload_parts_async(StepGroup& G, hipStream_t st, HostBuf& stage, hipEvent_t& ev) {
  if (ev) HIPCHK(hipEventSynchronize(ev));
  else HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  const size_t np = (size_t)G.S * G.Pl;
  CHK(stage.reserve(std::max<size_t>(1, np) * sizeof(PmPart)));
  PmPart* v = stage.as<PmPart>();
  for (uint32_t s = 0; s < G.S; ++s)
    for (uint32_t li = 0; li < G.Pl; ++li) {
      PmPart d = G.es[s]->parts[G.lp[li]].d;
      d.qv = G.qv.empty() ? nullptr : G.qv[s];
      v[(size_t)s * G.Pl + li] = d;
    }
  HIPCHK(hipMemcpyAsync(G.parts_d.p, v, np * sizeof(PmPart), hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(ev, st));
  G.gen.resize(G.S);
  for (uint32_t s = 0; s < G.S; ++s) G.gen[s] = G.es[s]->prep_gen;
  return 0;
}

static int drl_team_init(DrlTeam& T, pm_graph** gs, uint32_t S, uint32_t s0, const float* queries, uint64_t q, int k,
                         int step, int parallel, const DrlShape& sh) {
  T.gs = gs; T.S = S; T.s0 = s0;
  StepGroup& G = T.G;
  CHK(team_init(G, gs, S));
  hipStream_t st = G.c->stream;
  const pm_graph* g0 = gs[0];
  const Engine& e0 = g0->pir->e;
  const uint32_t P = (uint32_t)e0.P, m = (uint32_t)g0->m, n = sh.n, kcap = sh.kcap, dim = (uint32_t)g0->dim;
  T.nsub = S * P * sh.qn;
  if (!g0->dgraph->p) {   // the true neighbour lists (success count, start set) on the device, once per graph
    CHK(g0->dgraph->reserve(g0->n * m * 4));
    HIPCHK(hipMemcpy(g0->dgraph->p, g0->graph, g0->n * m * 4, hipMemcpyHostToDevice));
  }
  CHK(T.sess.reserve(S * sizeof(DrlSess)));
  CHK(T.dummy.reserve((uint64_t)S * P * 8));
  CHK(T.batch.reserve((uint64_t)S * n * 4));
  CHK(T.heap.reserve((uint64_t)S * kcap * 8));
  CHK(T.ktab.reserve((uint64_t)S * 2 * kcap * 8));
  CHK(T.knb.reserve((uint64_t)S * kcap * m * 4));
  CHK(T.kdist.reserve((uint64_t)S * kcap * 4));
  CHK(T.kid.reserve((uint64_t)S * kcap * 4));
  CHK(T.ctabp.reserve(S * 8));
  CHK(T.answers.reserve(std::max<uint64_t>(8, (uint64_t)S * q * k * 8)));
  // the step buffers of group_step for nsub sub-queries; the descriptor in them
  // (subs_d, sb_d) is the one the round kernels build
  CHK(G.buf.reserve(T.nsub, S * P, (G.maxPH + 63) / 64, pmk::step_match_blocks(G.maxPH), G.E));
  CHK(T.gid.reserve((uint64_t)T.nsub * 8));
  CHK(T.out.reserve(step_out_bytes(T.nsub, G.E)));
  CHK(T.allq.reserve(std::max<uint64_t>(4, (uint64_t)S * q * dim * 4)));
  CHK(T.part_bytes.reserve(P * 8));
  // host state -> device: search streams and counters, dummy counters, localCache indexes
  std::vector<DrlSess> hs(S);
  std::vector<uint64_t> dmy((uint64_t)S * P), ctp(S);
  for (uint32_t i = 0; i < S; ++i) {
    pm_graph* g = gs[i];
    Engine* e = &g->pir->e;
    hs[i] = DrlSess{g->rng.s, g->succ, 0, 0, 0, 0};
    for (uint32_t p = 0; p < P; ++p) dmy[(uint64_t)i * P + p] = e->parts[p].dummy_ctr;
    CHK(ensure_dev_cache(e, sh.cmask, st));
    ctp[i] = (uint64_t)(uintptr_t)e->dcache.p;
  }
  std::vector<uint32_t> sbv(S * P + 1);
  for (uint32_t j = 0; j <= S * P; ++j) sbv[j] = j * sh.qn;
  std::vector<double> pb(P);
  for (uint32_t p = 0; p < P; ++p) pb[p] = answer_bytes(e0.parts[p].d, G.E);
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipMemcpy(T.sess.p, hs.data(), S * sizeof(DrlSess), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(T.dummy.p, dmy.data(), dmy.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(T.ctabp.p, ctp.data(), S * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(G.buf.sb_d.p, sbv.data(), sbv.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(T.part_bytes.p, pb.data(), P * 8, hipMemcpyHostToDevice));
  if (q) HIPCHK(hipMemcpy(T.allq.p, queries + (uint64_t)s0 * q * dim, (uint64_t)S * q * dim * 4, hipMemcpyHostToDevice));
  if (G.c->timing >= 2) {   // each step's answer bytes and real sub-queries, counted by the round that builds it
    const uint64_t steps = q * (uint64_t)step;
    CHK(T.step_bytes.reserve(std::max<uint64_t>(8, steps * S * 8)));
    CHK(T.step_real.reserve(std::max<uint64_t>(4, steps * S * 4)));
    HIPCHK(hipMemsetAsync(T.step_bytes.p, 0, std::max<uint64_t>(8, steps * S * 8), st));   // accumulated by the rounds
    HIPCHK(hipMemsetAsync(T.step_real.p, 0, std::max<uint64_t>(4, steps * S * 4), st));
  }
  HIPCHK(hipEventCreateWithFlags(&T.ev_end, hipEventDisableTiming));
  if (getenv("PM_DRL_STAMPS")) {   // diagnostics: per-phase shader clocks of the MID rounds (printed at the end)
    CHK(T.stamps.reserve(16 * 8));
    HIPCHK(hipMemset(T.stamps.p, 0, 16 * 8));
  }
  DrlArgs& A = T.A;
  A.S = S; A.P = P; A.qn = sh.qn; A.n = n; A.m = m; A.parallel = (uint32_t)parallel; A.k = (uint32_t)k;
  A.E = G.E; A.dim = dim; A.kcap = kcap; A.cmask = sh.cmask; A.ns = G.ns; A.q = (uint32_t)q;
  A.N = g0->n; A.PS = e0.PS;
  A.vec16 = (G.E % 2 == 0 && dim % 4 == 0 && m % 4 == 0 && ((m / 4) & (m / 4 - 1)) == 0) ? 1u : 0u;
  A.hdr = T.out.as<PmOutHdr>();
  A.rows = (const uint64_t*)(T.out.as<char>() + (uint64_t)T.nsub * sizeof(PmOutHdr));
  A.subs = G.buf.subs_d.as<PmSub>(); A.gid = T.gid.as<uint64_t>();
  A.graph = g0->dgraph->as<uint32_t>();
  A.start_dist = G.start_dist.as<float>(); A.start_ids = G.start_ids.as<uint32_t>();
  A.sess = T.sess.as<DrlSess>(); A.dummy = T.dummy.as<uint64_t>(); A.batch = T.batch.as<uint32_t>();
  A.heap = T.heap.as<uint64_t>(); A.ktab = T.ktab.as<uint64_t>(); A.knb = T.knb.as<uint32_t>();
  A.kdist = T.kdist.as<float>(); A.kid = T.kid.as<uint32_t>(); A.ctab = T.ctabp.as<uint64_t*>();
  A.answers = T.answers.as<int64_t>(); A.part_bytes = T.part_bytes.as<double>();
  A.step_bytes = T.step_bytes.p ? T.step_bytes.as<double>() : nullptr;
  A.step_real = T.step_real.p ? T.step_real.as<uint32_t>() : nullptr;
  A.stamps = T.stamps.p ? T.stamps.as<uint64_t>() : nullptr;
  T.need.assign(S, 0);
  T.mt.assign(S, 0.0);
  return 0;
}

// One shared step of the device loop: the descriptor the last round kernel
// built, results into device memory.
static int drl_step(DrlTeam& T, const DrlShape& sh) {
  StepGroup& G = T.G;
  pm_ctx* c = G.c;
  const Engine* e0 = G.es[0];
  c->sample_now = c->sample_ctr++ % 7 == 0;   // timing level 3: group_step's sample
  PmStep S{};
  S.parts = G.parts_d.as<PmPart>();
  G.buf.fill(S, (G.maxPH + 63) / 64, pmk::step_match_blocks(G.maxPH));
  S.subs_h = S.subs;   // the descriptor is on the device already
  S.sb_h = S.sb;
  S.done = G.done.as<uint32_t>();
  S.db = e0->db->as<uint64_t>();
  S.q = nullptr;   // each partition's PmPart::qv
  step_out(S, T.out.p, T.nsub);
  S.E = G.E; S.dim = G.dim; S.nsub = T.nsub; S.np = T.S * G.Pl;
  S.np_live = S.np;
  S.args_valid = 0;
  S.token = next_token(G.token);
  step_read_window(S, e0->pf_off, e0->pf_len, G.E);
  S.rows_partial = 1;   // the rows stay on the device: no host diagnostic re-reads them
  const size_t before = c->launches.size();
  // bytes: every sub-query answered (patched with the round's exact count in timing runs)
  double ans_bytes = 0;
  for (uint32_t li = 0; li < G.Pl; ++li) ans_bytes += answer_bytes(e0->parts[G.lp[li]].d, G.E) * sh.qn * T.S;
  CHK(group_step_launch(G, S, sh.qn, T.nsub, ans_bytes));
  for (size_t i = before; i < c->launches.size(); ++i)
    if (c->launches[i].name == "answer" || c->launches[i].name == "match_resolve" || c->launches[i].name == "hint_match")
      T.tl.emplace_back(i, T.seq - 1);   // the step the last BEGIN / MID round built (drl_round advanced seq)
  c->host_add(HT_DEV_STEPS, 0.0);
  return 0;
}

static void drl_round(DrlTeam& T, uint32_t mode, uint64_t qi) {
  pm_ctx* c = T.G.c;
  DrlArgs A = T.A;
  A.mode = mode;
  A.qi = (uint32_t)qi;
  A.seq = T.seq;   // the step this round builds (BEGIN / MID)
  if (mode != DRL_END) T.seq++;
  c->timed_ext("team_round", 0, [&](pmk::PmEvents ev) { pmk::team_round(c->stream, A, ev); }, 2);
}

// Query qi of every team, enqueued round by round across the teams (so that
// teams whose streams share a hardware queue still interleave their rounds):
// per team the queries into qbuf, the start set's distances and BEGIN, then
// per round the shared step and the round kernel (MID, END after the last).
static int drl_begin(DrlTeam& T, uint64_t qi, uint64_t q) {
  StepGroup& G = T.G;
  hipStream_t st = G.c->stream;
  const uint32_t dim = G.dim;
  HIPCHK(hipMemcpy2DAsync(G.qbuf.p, (size_t)dim * 4, T.allq.as<float>() + qi * dim, (size_t)q * dim * 4,
                          (size_t)dim * 4, T.S, hipMemcpyDeviceToDevice, st));
  const uint64_t nrows = (uint64_t)T.S * G.ns;
  if (nrows)
    G.c->timed("l2_rows", (double)nrows * G.dim * 4, [&] {
      pmk::l2_rows(st, T.gs[0]->dvec->as<float>(), G.dim, nrows, G.start_ids.as<uint32_t>(), G.qbuf.as<float>(), G.dim,
                   G.start_dist.as<float>(), G.ns);
    });
  drl_round(T, DRL_BEGIN, qi);
  return 0;
}
static int drl_query_all(std::vector<std::unique_ptr<DrlTeam>>& teams, const DrlShape& sh, uint64_t qi, uint64_t q,
                         int step) {
  for (auto& t : teams) CHK(drl_begin(*t, qi, q));
  for (int r = 0; r < step; ++r)
    for (auto& t : teams) {
      CHK(drl_step(*t, sh));
      drl_round(*t, r + 1 == step ? DRL_END : DRL_MID, qi);
    }
  HIPCHK(hipGetLastError());
  for (auto& t : teams) {
    for (uint32_t i = 0; i < t->S; ++i) {   // the host's deterministic mirrors of the rounds (bq_tail, gvi_pre)
      pm_graph* g = t->gs[i];
      Engine* e = &g->pir->e;
      e->FBN += (uint64_t)step * (sh.n / e->B);
      e->QMIP += (uint64_t)step * sh.qn;
      g->total += (uint64_t)step * sh.n;
    }
    t->G.c->host_add(HT_DEV_QUERIES, (double)t->S);
  }
  return 0;
}

// Device state -> host at the end of the call: answers, search streams and
// counters, dummy counters, FinishedQueryNum; the timed launches' bytes.
static int drl_team_finish(DrlTeam& T, uint64_t q, int k, int64_t* answers) {
  StepGroup& G = T.G;
  HIPCHK(hipStreamSynchronize(G.c->stream));
  const uint32_t S = T.S, P = (uint32_t)G.es[0]->P;
  if (q) HIPCHK(hipMemcpy(answers + (uint64_t)T.s0 * q * k, T.answers.p, (uint64_t)S * q * k * 8, hipMemcpyDeviceToHost));
  std::vector<DrlSess> hs(S);
  std::vector<uint64_t> dmy((uint64_t)S * P);
  HIPCHK(hipMemcpy(hs.data(), T.sess.p, S * sizeof(DrlSess), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(dmy.data(), T.dummy.p, dmy.size() * 8, hipMemcpyDeviceToHost));
  std::vector<uint32_t> fq(P);
  for (uint32_t i = 0; i < S; ++i) {
    pm_graph* g = T.gs[i];
    Engine* e = &g->pir->e;
    g->rng.s = hs[i].rng;
    g->succ = hs[i].succ;
    HIPCHK(hipMemcpy(fq.data(), e->fqn.p, P * 4, hipMemcpyDeviceToHost));
    for (uint32_t p = 0; p < P; ++p) {
      e->parts[p].dummy_ctr = dmy[(uint64_t)i * P + p];
      e->parts[p].fqn = fq[p];
    }
  }
  if (T.stamps.p) {
    uint64_t st[16];
    HIPCHK(hipMemcpy(st, T.stamps.p, sizeof st, hipMemcpyDeviceToHost));
    if (st[15])
      fprintf(stderr, "[pm] team_round MID phases (shader clocks per launch, %lu launches): load %.0f respond %.0f decode %.0f "
              "[ballot %.0f known %.0f rows %.0f push %.0f fence %.0f] pop+gather %.0f bucket %.0f store %.0f\n",
              (unsigned long)st[15], st[1] / (double)st[15], st[2] / (double)st[15], st[3] / (double)st[15],
              st[8] / (double)st[15], st[9] / (double)st[15], st[10] / (double)st[15], st[11] / (double)st[15],
              st[4] / (double)st[15], st[5] / (double)st[15], st[6] / (double)st[15], st[7] / (double)st[15]);
  }
  pm_ctx* c = G.c;
  if (!T.tl.empty() && T.step_bytes.p) {   // the timed steps' exact answer bytes / real sub-queries
    std::vector<double> by((uint64_t)T.seq * S);
    std::vector<uint32_t> nr((uint64_t)T.seq * S);
    HIPCHK(hipMemcpy(by.data(), T.step_bytes.p, by.size() * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(nr.data(), T.step_real.p, nr.size() * 4, hipMemcpyDeviceToHost));
    for (auto& [idx, sq] : T.tl) {
      if (idx >= c->launches.size() || sq >= T.seq) continue;
      double b = 0, r = 0;
      for (uint32_t i = 0; i < S; ++i) { b += by[(uint64_t)sq * S + i]; r += nr[(uint64_t)sq * S + i]; }
      if (c->launches[idx].name == "answer") c->launches[idx].bytes = b;
      else c->launches[idx].bytes = r * G.maxPH;
    }
  }
  return 0;
}

static int run_batched_dev_body(pm_graph** gs, uint32_t S, const float* queries, uint64_t q, int k, int step,
                                int parallel, uint32_t NG, int64_t* answers, double* mt_out, const DrlShape& sh,
                                std::vector<std::unique_ptr<DrlTeam>>& teams) {
  std::vector<StreamSwap> swaps(NG);   // (destroyed after the teams: drained, restored)
  struct Release {
    std::vector<std::unique_ptr<DrlTeam>>& t;
    ~Release() { for (auto& x : t) if (x->gs) team_release(x->gs, x->S); }
  } release{teams};
  for (uint32_t g = 0; g < NG; ++g) {
    const uint32_t s0 = (uint32_t)((uint64_t)S * g / NG), s1 = (uint32_t)((uint64_t)S * (g + 1) / NG);
    teams.emplace_back(new DrlTeam());
    CHK(drl_team_init(*teams.back(), gs + s0, s1 - s0, s0, queries, q, k, step, parallel, sh));
    swaps[g].swap_in(teams.back()->G.c, team_stream(teams.back()->G.c->device, g));
  }
  // Maintenance launch sets, timed by events around them on the leader's stream
  struct PrepSet { hipEvent_t a = nullptr, b = nullptr; std::vector<std::pair<DrlTeam*, uint32_t>> members; };
  std::vector<PrepSet> sets;
  struct SetsRelease {
    std::vector<PrepSet>& v;
    ~SetsRelease() { for (auto& x : v) { if (x.a) (void)hipEventDestroy(x.a); if (x.b) (void)hipEventDestroy(x.b); } }
  } sets_release{sets};
  for (uint64_t qi = 0; qi < q; ++qi) {
    if ((int64_t)g_fault_drl_query.load() == (int64_t)qi) return fail(PM_EHIP, "injected fault (fault_drl_query)");
    CHK(drl_query_all(teams, sh, qi, q, step));
    // the harness's maintenance trigger (private-search.go:226-232) per session:
    // the triggered clients of every team as ONE launch set after the query
    std::vector<Engine*> who;
    std::vector<double*> mts;
    std::vector<DrlTeam*> involved;
    for (auto& t : teams) {
      bool any = false;
      for (uint32_t i = 0; i < t->S; ++i) {
        Engine* e = &t->gs[i]->pir->e;
        t->need[i] = e->FBN + (uint64_t)step * (uint64_t)parallel + 10 >= e->Support;
        if (t->need[i]) { who.push_back(e); mts.push_back(&t->mt[i]); any = true; }
      }
      if (any) involved.push_back(t.get());
    }
    if (who.empty()) continue;
    // ONE launch set of every triggered client, on the first involved team's
    // stream after every involved team's query; nothing on the host waits for
    // it (the other teams keep running what is queued), and the involved
    // teams' next rounds wait for it on the device
    DrlTeam* L = involved[0];
    hipStream_t const sl = L->G.c->stream;
    for (DrlTeam* t : involved)
      if (t != L) {
        HIPCHK(hipEventRecord(t->ev_end, t->G.c->stream));
        HIPCHK(hipStreamWaitEvent(sl, t->ev_end, 0));
      }
    sets.emplace_back();
    PrepSet& ps = sets.back();
    HIPCHK(hipEventCreate(&ps.a));
    HIPCHK(hipEventCreate(&ps.b));
    HIPCHK(hipEventRecord(ps.a, sl));
    CHK(prep_clients(L->G.c, L->prep_buf, L->G.lp, who, nullptr, &L->prep_stage, &L->prep_stage_ev));
    for (DrlTeam* t : involved) {   // the new keys into the team's parts; the emptied localCache indexes
      CHK(group_upload_parts_async(t->G, sl, t->parts_stage, t->parts_stage_ev));
      for (uint32_t i = 0; i < t->S; ++i)
        if (t->need[i]) {
          CHK(ensure_dev_cache(&t->gs[i]->pir->e, sh.cmask, sl));
          ps.members.emplace_back(t, i);
        }
    }
    HIPCHK(hipEventRecord(ps.b, sl));
    for (DrlTeam* t : involved)
      if (t != L) HIPCHK(hipStreamWaitEvent(t->G.c->stream, ps.b, 0));
  }
  for (auto& t : teams) CHK(drl_team_finish(*t, q, k, answers));
  for (PrepSet& ps : sets) {   // each triggered client's maintenance time: its launch set's span on the GPU
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ps.a, ps.b));
    for (auto& [t, i] : ps.members) {
      t->mt[i] += ms / 1e3;
      record_stats(&t->gs[i]->pir->e, ms / 1e3);   // PreprocessingTime: the set's GPU span
    }
  }
  for (auto& t : teams)
    for (uint32_t i = 0; i < t->S; ++i) mt_out[t->s0 + i] = t->mt[i];
  return 0;
}

// The device loop; on a failure after the teams started, their streams are
// drained (nothing left running on the buffers being freed) and every session
// is marked lost: its host mirrors were advanced for queries whose device state
// was never read back.
static int run_batched_dev(pm_graph** gs, uint32_t S, const float* queries, uint64_t q, int k, int step, int parallel,
                           uint32_t NG, int64_t* answers, double* mt_out, const DrlShape& sh) {
  std::vector<std::unique_ptr<DrlTeam>> teams;
  const int rc = run_batched_dev_body(gs, S, queries, q, k, step, parallel, NG, answers, mt_out, sh, teams);
  if (rc == 0) return 0;
  const std::string why = pm_last_error();
  for (auto& t : teams)
    if (t && t->G.c) (void)hipStreamSynchronize(t->G.c->stream);
  (void)hipDeviceSynchronize();
  for (uint32_t i = 0; i < S; ++i) gs[i]->lost = "device loop failed: " + why;
  return fail(rc, why);
}

extern "C" int pm_search_loop_batched(pm_graph** gs, uint32_t S, const float* queries, uint64_t q, int k, int step,
                                      int parallel, uint32_t ngroups, uint32_t nthreads, int64_t* answers,
                                      double* wall_s, double* online_s, double* maint_s) {
  if (!gs || !S || (!queries && q) || (!answers && q)) return fail(PM_EINVAL, "NULL argument");
  for (uint32_t i = 0; i < S; ++i) {
    if (!gs[i] || !gs[i]->pir || gs[i]->nonprivate) return fail(PM_EINVAL, "sessions must be preprocessed private graphs");
    CHK(check_session(gs[i]));
    const Engine& a = gs[0]->pir->e;
    const Engine& b = gs[i]->pir->e;
    if (a.db.get() != b.db.get() || a.P != b.P || a.E != b.E || gs[i]->dim != gs[0]->dim || gs[i]->m != gs[0]->m ||
        b.nshards != 1 || gs[i]->ctx->device != gs[0]->ctx->device)
      return fail(PM_EINVAL, "batched sessions must be clients of one server DB on one device");
    for (uint32_t j = 0; j < i; ++j)
      if (gs[j] == gs[i] || gs[j]->ctx == gs[i]->ctx) return fail(PM_EINVAL, "sessions need distinct graphs and contexts");
  }
  // teams: sessions split into `ngroups` lock-step groups with their own step
  // streams, run concurrently (one group's shared step on the GPU while the
  // others' searches run on the host); threads split evenly
  const uint32_t NG = std::max(1u, std::min(ngroups ? ngroups : 1u, S));
  const uint32_t TT = std::max(NG, nthreads ? nthreads : std::min<uint32_t>(S, 16u));
  std::vector<double> mt(S, 0.0);
  std::vector<int> rc(NG, 0);
  std::vector<std::string> msg(NG);
  std::vector<std::thread> teams;
  const float* qbase = queries;
  auto t0 = Clock::now();
  DrlShape sh;
  if (drl_plan(gs, S, q, k, step, parallel, &sh)) {   // every round on the GPU (run_batched_dev)
    CHK(run_batched_dev(gs, S, queries, q, k, step, parallel, NG, answers, mt.data(), sh));
  } else {
    static const int pool = [] { const char* e = getenv("PM_BATCH_POOL"); return e ? atoi(e) : 1; }();
    if (pool && NG > 1) {   // the pooled workers (run_batched_pool); one team: the workers serve it alone anyway
      CHK(run_batched_pool(gs, S, queries, q, k, step, parallel, NG, TT, answers, mt.data()));
    } else {
      for (uint32_t g = 0; g < NG; ++g) {
        const uint32_t s0 = (uint32_t)((uint64_t)S * g / NG), s1 = (uint32_t)((uint64_t)S * (g + 1) / NG);
        const uint32_t Tg = std::max(1u, std::min(s1 - s0, (uint32_t)((uint64_t)TT * (g + 1) / NG - (uint64_t)TT * g / NG)));
        teams.emplace_back([&, g, s0, s1, Tg] {
          if (hipSetDevice(gs[0]->ctx->device) != hipSuccess) { rc[g] = PM_EHIP; msg[g] = "hipSetDevice"; return; }
          rc[g] = run_batched_team(gs + s0, s1 - s0, qbase + (uint64_t)s0 * q * gs[0]->dim, q, k, step, parallel, Tg,
                                   answers + (uint64_t)s0 * q * (uint64_t)k, mt.data() + s0);
          if (rc[g]) msg[g] = pm_last_error();
        });
      }
      for (auto& t : teams) t.join();
      for (uint32_t g = 0; g < NG; ++g)
        if (rc[g]) return fail(rc[g], "group " + std::to_string(g) + ": " + msg[g]);
    }
  }
  const double wall = std::chrono::duration<double>(Clock::now() - t0).count();
  if (wall_s) *wall_s = wall;
  for (uint32_t s = 0; s < S; ++s) {
    if (online_s) online_s[s] = wall - mt[s];
    if (maint_s) maint_s[s] = mt[s];
  }
  return 0;
}

// Words of one team's records in pm_search_loop_sharded: sessions x (parallel
// x m) ids x W, W = the row words holding the neighbour list + 1.
extern "C" uint64_t pm_sharded_record_words(pm_graph* g, uint32_t sessions, int parallel) {
  if (!g || parallel <= 0) return 0;
  const uint64_t w0 = g->dim * 4 / 8, w1 = (g->dim * 4 + g->m * 4 + 7) / 8;
  return (uint64_t)sessions * (uint64_t)parallel * g->m * (w1 - w0 + 1) + 1;   // + the error word
}

// The batched serving loop over a sharded graph DB (every rank calls it with
// its own shard's sessions, the same seeds and queries).  Teams are
// pm_search_loop_batched's; each shared step ends in ONE combine of the team's
// records (see group_exchange).  combine NULL: no exchange (one shard holds
// every partition), or model_peers (synthetic graphs): the partitions of the
// other shards are answered from the graph's spec.  team_bufs (NULL: the
// library allocates): one device buffer per team of pm_sharded_record_words
// words, the tensors a torch.distributed combine all-reduces in place.
extern "C" int pm_search_loop_sharded(pm_graph** gs, uint32_t S, const float* queries, uint64_t q, int k, int step,
                                      int parallel, uint32_t ngroups, uint32_t nthreads, pm_combine_fn combine,
                                      void* user, uint64_t* const* team_bufs, int model_peers, int64_t* answers,
                                      double* wall_s, double* online_s, double* maint_s) {
  if (!gs || !S || (!queries && q) || (!answers && q)) return fail(PM_EINVAL, "NULL argument");
  for (uint32_t i = 0; i < S; ++i) {
    if (!gs[i] || !gs[i]->pir || gs[i]->nonprivate) return fail(PM_EINVAL, "sessions must be preprocessed private graphs");
    CHK(check_session(gs[i]));
    const Engine& a = gs[0]->pir->e;
    const Engine& b = gs[i]->pir->e;
    if (a.db.get() != b.db.get() || a.P != b.P || a.E != b.E || gs[i]->dim != gs[0]->dim || gs[i]->m != gs[0]->m ||
        b.shard != a.shard || b.nshards != a.nshards || gs[i]->ctx->device != gs[0]->ctx->device)
      return fail(PM_EINVAL, "sharded sessions must be clients of one shard's server DB on one device");
    for (uint32_t j = 0; j < i; ++j)
      if (gs[j] == gs[i] || gs[j]->ctx == gs[i]->ctx) return fail(PM_EINVAL, "sessions need distinct graphs and contexts");
  }
  if (model_peers && !gs[0]->synth) return fail(PM_EINVAL, "modelled peers need the synthetic graph (its rows are computable)");
  if (model_peers && combine) return fail(PM_EINVAL, "pass a combine or model_peers, not both");
  if (gs[0]->pir->e.nshards > 1 && !combine && !model_peers)
    return fail(PM_EINVAL, "a sharded graph needs a combine (or model_peers)");
  if (gs[0]->m > 64) return fail(PM_EINVAL, "sharded search: m <= 64");
  const uint32_t NG = std::max(1u, std::min(ngroups ? ngroups : 1u, S));
  const uint32_t TT = std::max(NG, nthreads ? nthreads : std::min<uint32_t>(S, 16u));
  ShardComb comb;
  comb.fn = combine;
  comb.user = user;
  comb.model_peers = model_peers != 0;
  comb.NG = NG;
  comb.bufs = team_bufs;
  std::vector<double> mt(S, 0.0);
  std::vector<int> rc(NG, 0);
  std::vector<std::string> msg(NG);
  std::vector<std::thread> teams;
  auto t0 = Clock::now();
  for (uint32_t g = 0; g < NG; ++g) {
    const uint32_t s0 = (uint32_t)((uint64_t)S * g / NG), s1 = (uint32_t)((uint64_t)S * (g + 1) / NG);
    const uint32_t Tg = std::max(1u, std::min(s1 - s0, (uint32_t)((uint64_t)TT * (g + 1) / NG - (uint64_t)TT * g / NG)));
    teams.emplace_back([&, g, s0, s1, Tg] {
      if (hipSetDevice(gs[0]->ctx->device) != hipSuccess) { rc[g] = PM_EHIP; msg[g] = "hipSetDevice"; return; }
      rc[g] = run_batched_team(gs + s0, s1 - s0, queries + (uint64_t)s0 * q * gs[0]->dim, q, k, step, parallel, Tg,
                               answers + (uint64_t)s0 * q * (uint64_t)k, mt.data() + s0, &comb, g);
      if (rc[g]) { msg[g] = pm_last_error(); comb.abort.store(true); }
    });
  }
  for (auto& t : teams) t.join();
  const double wall = std::chrono::duration<double>(Clock::now() - t0).count();
  for (uint32_t g = 0; g < NG; ++g)
    if (rc[g]) return fail(rc[g], "group " + std::to_string(g) + ": " + msg[g]);
  if (wall_s) *wall_s = wall;
  for (uint32_t s = 0; s < S; ++s) {
    if (online_s) online_s[s] = wall - mt[s];
    if (maint_s) maint_s[s] = mt[s];
  }
  return 0;
}
