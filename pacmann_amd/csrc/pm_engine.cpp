// pm_engine.cpp — the PianoPIR / SimpleBatchPianoPIR engine of libpacmann.so:
// device-resident DB, hints and client state, the batched step with its
// completion and result publication, and the pm_pir_* / pm_batchpir_* boundary
// of include/pacmann.h.  Needs pm_ctx.cpp only.
#include "pm_engine.h"

static void derive_key(uint64_t seed, uint64_t part, uint64_t epoch, uint8_t key[16]) {
  uint64_t r1 = hash4(seed, DOM_KEY, part, epoch, 0), r2 = hash4(seed, DOM_KEY, part, epoch, 1);
  memcpy(key, &r1, 8);
  memcpy(key + 8, &r2, 8);
}

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

namespace pmh {
int engine_create(pm_ctx* ctx, Engine* g, uint64_t N, uint64_t Ebytes, uint64_t B,
                         const uint64_t* rawDB, uint64_t F, uint64_t seed, bool batch,
                         uint32_t shard, uint32_t nshards, const Engine* server,
                         const DbGen* gen, uint32_t coord_words, bool remote) {
  if (nshards == 0 || shard >= nshards) return fail(PM_EINVAL, "shard must be < nshards");
  if (!ctx) return fail(PM_EINVAL, "ctx is NULL");
  if (!rawDB && N && !server && !gen && !remote) return fail(PM_EINVAL, "rawDB is NULL");
  if (gen && gen->kind == 1 && (uint64_t)(gen->dim + gen->m) * 4 != Ebytes)
    return fail(PM_EINVAL, "graph entry size must be 4 * (dim + m)");
  if (server && server->ctx->device != ctx->device) return fail(PM_EINVAL, "a client shares the server DB of its own device only");
  if (N == 0) return fail(PM_EINVAL, "DBSize must be > 0");
  if (Ebytes < 8) return fail(PM_EINVAL, "DBEntryByteNum must be >= 8");
  HIPCHK(hipSetDevice(ctx->device));
  g->ctx = ctx; g->is_batch = batch;
  g->N = N; g->Ebytes = Ebytes; g->E = Ebytes / 8; g->F = F; g->seed = seed;
  g->remote = remote;
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
  else if (!remote) CHK(g->db->reserve(std::max<uint64_t>(8, off_db * g->E * 8)));   // a remote client holds no rows
  for (uint32_t i : server || remote ? std::vector<uint32_t>{} : g->owned_list) {
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
  // k_prep_fold_rot (CS 512 and 1,024 shapes; pm_set_option "fold_rot" 0 or
  // PM_FOLD_ROT=0 disables it).  It is skipped, and the fold reads the rows
  // themselves (k_prep_fold_pipe), when it would take more than a quarter of
  // the device memory still free, or for a client of a server without one.
  // The option is read here and nowhere later: off_img decides the table
  // allocation below and the fold form of every preprocessing of this engine.
  // A graph DB (coord_words: the 32-bit coordinate words that begin every
  // entry; 0 for a bare PIR engine, which never qualifies) whose coordinates
  // all have zero low halves, e.g. f32 holding SIFT's bytes, gets the packed
  // image (FOLD_ROT512P): one reduction over the rows decides, once, since the
  // DB does not change.  A client takes its server's image and decision.
  // The same property lets the pair answer gather packed rows (the row image
  // below), so the reduction runs once if either image wants it.
  uint64_t off_img = 0;
  const bool fold_img = !remote && !g->owned_list.empty() && pmk::fold_image_ok(g->minCS, g->maxCS, (uint32_t)g->E);
  const uint32_t want_npk = !server && fold_img ? pmk::fold_pack_slices(g->minCS, g->maxCS, (uint32_t)g->E, coord_words) : 0;
  const uint32_t want_apk = !server && !remote && !g->owned_list.empty() ? pmk::answer_pack_segs((uint32_t)g->E, coord_words) : 0;
  // The same pass looks at the other bits that are the same in every row of
  // such a DB (the coordinates' sign and copied exponent bits, the ids' bits
  // above 19): where they allow a bit-packed image of fewer slices, the server
  // builds that one instead (FOLD_ROT512Q, pmk::fold_bits_form).
  bool low_zero = false;
  uint32_t row_bits = 0;
  if (want_npk || want_apk) {
    DevBuf flag;
    CHK(flag.reserve(64));
    row_bits = pmk::row_bits_or(ctx->stream, g->db->as<uint64_t>(), off_db, (uint32_t)g->E, coord_words, flag.as<uint32_t>());
    low_zero = !(row_bits & pmk::kRowLowHalf);
    HIPCHK(hipGetLastError());
  }
  if (fold_img) {
    if (server) { g->img_npk = server->img_npk; g->img_bits = server->img_bits; }
    else if (low_zero) {
      g->img_bits = pmk::fold_bits_form((uint32_t)g->E, coord_words, want_npk, row_bits);
      g->img_npk = g->img_bits ? 0 : want_npk;
    }
    for (uint32_t i : g->owned_list) {
      PmPart& d = g->parts[i].d;
      d.img = (const uint64_t*)(uintptr_t)off_img;
      off_img += pmk::fold_image_words(d.SS, (uint32_t)g->E, (uint32_t)g->maxCS, g->img_npk, g->img_bits);
    }
    size_t free_b = 0, total_b = 0;
    if (!server && hipMemGetInfo(&free_b, &total_b) == hipSuccess && off_img * 8 > free_b / 4) {
      for (uint32_t i : g->owned_list) g->parts[i].d.img = nullptr;
      off_img = 0;
    } else if (server && !server->img->p) {   // the server went without one
      for (uint32_t i : g->owned_list) g->parts[i].d.img = nullptr;
      off_img = 0;
    }
    if (!off_img) g->img_npk = g->img_bits = 0;
  }
  if (off_img) {
    if (server) {
      g->img = server->img;
    } else {
      CHK(g->img->reserve(off_img * 8));
      for (uint32_t i : g->owned_list) {
        const PmPart& d = g->parts[i].d;
        pmk::fold_image(ctx->stream, g->img->as<uint64_t>() + (uintptr_t)d.img, g->db->as<uint64_t>() + d.row0 * g->E,
                        d.N, d.SS, (uint32_t)g->E, (uint32_t)g->maxCS, g->img_npk, g->img_bits);
      }
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(ctx->stream));
    }
  }
  // the packed row image of the pair answer (k_answer_p5k / k_answer_pk): the
  // owned rows in db's order, without the coordinates' zero low halves.  Built
  // once by the server under the fold image's memory rule; db stays for every
  // other reader.  A client takes its server's image and decision.
  if (server) {
    g->apk = server->apk; g->apk_nseg = server->apk_nseg; g->apk_cseg = server->apk_cseg;
  } else if (want_apk && low_zero) {
    const uint64_t bytes = off_db * want_apk * 16;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes <= free_b / 4) {
      CHK(g->apk->reserve(bytes));
      pmk::answer_pack_image(ctx->stream, g->apk->as<uint64_t>(), g->db->as<uint64_t>(), off_db, (uint32_t)g->E, coord_words);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(ctx->stream));
      g->apk_nseg = want_apk; g->apk_cseg = coord_words / 8;
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
  // (nor for a remote client: the streamed fold reads tabT)
  const bool need_tab = !remote && pmk::fold_needs_tab(g->minCS, g->maxCS, (uint32_t)g->E, off_img != 0);
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
}  // namespace pmh

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

namespace pmh {
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
int ensure_host_cache(Engine* g) {
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

int engine_prep_host(Engine* g, uint64_t p0, uint64_t p1, std::vector<uint64_t>& todo,
                            hipStream_t st) {
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
int engine_prep_launch(pm_ctx* c, const Engine* g, const PmPart* dp, int np, const PmPart* host_parts,
                              uint32_t clients, bool sync) {
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
    // have_img: whether this engine was created with a fold image (its own or its
    // server's); with the shape it fixes the fold form for the engine's lifetime
    int kind = pmk::FOLD_GATHER;
    c->timed("prep_fold", fold, [&] { kind = pmk::prep_fold(st, dp, np, g->maxH, g->db->as<uint64_t>(), (uint32_t)g->E, g->minCS,
                                                      g->maxCS, g->zero16.as<uint64_t>(), clients, g->img->p != nullptr, minH,
                                                      g->img_npk, g->img_bits); });
    if (kind == pmk::FOLD_ROT512 || kind == pmk::FOLD_ROT512P || kind == pmk::FOLD_ROT512Q || kind == pmk::FOLD_ROT1024) {
      c->host_add(kind == pmk::FOLD_ROT512 ? HT_FOLD_ROT512 : kind == pmk::FOLD_ROT512P ? HT_FOLD_ROT512P
                  : kind == pmk::FOLD_ROT512Q ? HT_FOLD_ROT512Q : HT_FOLD_ROT1024,
                  kind == pmk::FOLD_ROT512Q ? (double)pmk::fold_bits_slices(g->img_bits, (uint32_t)g->E) : 0.0);
    } else {
      c->host_add(HT_FOLD_OTHER, 0.0);
      c->host_add(kind == pmk::FOLD_PIPE ? HT_FOLD_PIPE : kind == pmk::FOLD_BLK ? HT_FOLD_BLK : HT_FOLD_GATHER, 0.0);
    }
    if (side) HIPCHK(hipStreamWaitEvent(st, c->side_ev[1], 0));
    else c->timed("prep_repl", repl, [&] { pmk::prep_repl(st, dp, np, g->maxRepl, g->db->as<uint64_t>(), (uint32_t)g->E); });
  }
  HIPCHK(hipGetLastError());
  if (sync) HIPCHK(hipStreamSynchronize(st));
  return 0;
}
}  // namespace pmh
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

namespace pmh {
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
int wait_done(pm_ctx* sc, uint64_t seq) {
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
int poll_done(pm_ctx* sc, uint64_t seq, bool* ready) {
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

int wait_step(pm_ctx* c, const PmOutHdr* hdr, uint32_t nsub, uint32_t token, const char* rows,
                     size_t row_bytes, size_t pf_off, size_t pf_len, uint64_t seq, pm_ctx* sc) {
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
}  // namespace pmh

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

namespace pmh {
// The host side of a published step for one engine whose sub-queries are
// [base, base + nsub) of the step (base > 0 when several clients shared the
// step, pm_search_loop_batched): result pointers, FinishedQueryNum and
// localCache mirrors (pir.go:469-470), in-step cache hits copied from the
// earlier response (their reference is a step-wide sub-query index).
void post_results(Engine* g, PmOutHdr* hdr, uint64_t* rows, uint32_t nsub, uint32_t base,
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

#if defined(PM_STEP_STAMPS) || defined(PM_MR_STAMPS) || defined(PM_ANSWER_STAMPS)
// Stamp builds: one launch's stamps.  begin: when the environment names a file `f` (and, with
// `first`, for the run's first 40 such launches only: the file's size), S.stamps
// = `words` zeroed words; end: `hdr` and the words appended to the file.
struct LaunchStamps {
  const char* file = nullptr;
  uint64_t words = 0;
  int begin(const char* f, std::atomic<int>* first, hipStream_t st, StepBufs& B, PmStep& S, uint64_t n) {
    if (!f || (first && first->fetch_add(1) >= 40)) return 0;
    CHK(B.stamps.reserve(n * 8));
    HIPCHK(hipMemsetAsync(B.stamps.p, 0, n * 8, st));
    S.stamps = B.stamps.as<uint64_t>();
    file = f; words = n;
    return 0;
  }
  int end(hipStream_t st, const StepBufs& B, PmStep& S, const void* hdr, size_t hdr_bytes) {
    if (!file) return 0;
    S.stamps = nullptr;
    return dump_stamps(st, file, hdr, hdr_bytes, B.stamps, words);
  }
};
#endif

// The kernels of one step whose descriptor S is complete, as pmk::step_plan
// chooses them for `shape`: k_step alone, or the hint search + resolution (one
// launch, k_match_resolve*, where the shapes hold), the split gather for wide
// sets and the answer.  Applies the plan's fields to S, reserves what it asks
// for, times and counts every launch by its form ("host_path_*").
// after_resolve (if any) runs between the resolution and the gather / answer.
int step_chain(pm_ctx* c, StepBufs& B, PmStep& S, const pmk::StepShape& shape, uint32_t nreal, double ans_bytes,
               const std::function<int()>& after_resolve) {
  hipStream_t st = c->stream;
  if (shape.desc_shared != (S.subs == S.subs_h && S.sb == S.sb_h))
    return fail(PM_EINVAL, "step_chain: the descriptor is not where the step's shape says");
  const pmk::StepPlan plan = pmk::step_plan(shape, pmk::step_opts());
  S.args_valid = shape.args_valid ? 1u : 0u;
  S.nsplit = plan.nsplit; S.qw = plan.qw; S.np_live = plan.np_live; S.cblk = plan.cblk; S.nhelp = plan.nhelp; S.no_guess = plan.no_guess;
  S.help_spoil = plan.help_spoil;
  const uint32_t nsub = S.nsub;
  if (plan.qset) {
    CHK(B.qset.reserve((uint64_t)nsub * plan.qw * 2));
    S.qset = B.qset.as<uint16_t>();
  }
  if (plan.nsplit > 1) {
    CHK(B.part_x.reserve((uint64_t)nsub * plan.nsplit * (S.E & ~3u) * 8));
    S.part_x = B.part_x.as<uint64_t>();
  }
  const bool fused = plan.at[pmk::STAGE_FUSED].form >= 0;
  if (fused) {
    if (plan.nhelp && !B.helpg.p) {   // the helpers' hand-off granules, on first use (token 0 never marks a step)
      const size_t nh = (size_t)kArgSubs * kStepHelpMax * kHelpGran * 8;
      CHK(B.helpg.reserve(nh));
      HIPCHK(hipMemsetAsync(B.helpg.p, 0, nh, st));
    }
    S.helpg = B.helpg.as<uint64_t>();
  }
  B.spec_nsub = 0;
  if (fused && c->step_spec) {   // k_step's speculation record (pm_batchpir_step_spec), zeroed: 0 = never stored
    CHK(B.specrec.reserve(kArgSubs * 4));
    HIPCHK(hipMemsetAsync(B.specrec.p, 0, kArgSubs * 4, st));
    S.specrec = B.specrec.as<uint32_t>();
    B.spec_nsub = nsub;
  }
  // Timing level 2: the kernels carry their events in their own dispatch packets.
  auto run = [&](int stage, const char* name, double bytes) {
    const int form = plan.at[stage].form;
    if (form < 0) return;
    c->timed_ext(name, bytes, [&](pmk::PmEvents ev) { pmk::step_launch(st, S, plan, stage, ev); }, 2);
    c->host_add(pm_ctx::step_counter(stage, form), stage == pmk::STAGE_FUSED ? plan.nhelp : 0.0);   // k_step: its nhelp
    if (pmk::step_answer_packed(S, plan, stage)) c->host_add(HT_ANSWER_PACKED, 0.0);
  };
#ifdef PM_STEP_STAMPS
  LaunchStamps ss;   // {grid, nsub, cblk, np} + grid x 8 stamps per k_step (PM_STAMP_FILE)
  const uint32_t sh[4] = {plan.at[pmk::STAGE_FUSED].gx, nsub, pmk::step_match_blocks(shape.maxPH), S.np};
  if (fused) CHK(ss.begin(getenv("PM_STAMP_FILE"), nullptr, st, B, S, (uint64_t)sh[0] * 8));
#endif
  run(pmk::STAGE_FUSED, "step", ans_bytes);
#ifdef PM_STEP_STAMPS
  CHK(ss.end(st, B, S, sh, sizeof sh));
#endif
#ifdef PM_MR_STAMPS
  LaunchStamps ms;   // {np} + np x 8 stamps per k_match_resolve* (PM_MR_STAMPS)
  static std::atomic<int> mr_steps{0};
  const uint64_t mh = S.np;
  if (plan.at[pmk::STAGE_MR].form >= 0) CHK(ms.begin(getenv("PM_MR_STAMPS"), &mr_steps, st, B, S, mh * 8));
#endif
  run(pmk::STAGE_MR, "match_resolve", (double)nreal * shape.maxPH);
#ifdef PM_MR_STAMPS
  CHK(ms.end(st, B, S, &mh, sizeof mh));
#endif
  run(pmk::STAGE_MATCH, "hint_match", (double)nreal * shape.maxPH);
  run(pmk::STAGE_RESOLVE, "resolve", 0);
  if (after_resolve) {
    const int r = after_resolve();
    if (r == kChainStop) return 0;   // the client role: the answer is another call's (pm_batchpir_client_finish)
    CHK(r);
  }
  run(pmk::STAGE_GATHER, "gather", ans_bytes);
#ifdef PM_ANSWER_STAMPS
  LaunchStamps as;   // {nsub} + nsub x 8 stamps per answer kernel (PM_ANSWER_STAMPS)
  static std::atomic<int> ans_steps{0};
  const uint64_t ah = nsub;
  if (!fused) CHK(as.begin(getenv("PM_ANSWER_STAMPS"), &ans_steps, st, B, S, ah * 8));
#endif
  run(pmk::STAGE_ANSWER, "answer", plan.nsplit > 1 ? 0 : ans_bytes);
#ifdef PM_ANSWER_STAMPS
  CHK(as.end(st, B, S, &ah, sizeof ah));
#endif
  return 0;
}

// The descriptor of the engine's own step over g->subs / g->sb (at least one
// sub-query), its scratch reserved, and what pmk::step_plan chooses from.
static int step_setup(Engine* g, const float* q_dev, uint32_t dim, PmStep& S, pmk::StepShape& shape, uint32_t& nreal,
                      double& ans_bytes) {
  pm_ctx* c = g->ctx;
#ifdef PM_STAMPS
  hipStream_t st = c->stream;
#endif
  const uint32_t nsub = (uint32_t)g->subs.size();
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
  S = PmStep{};
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
  g->step_db(S);
  S.q = q_dev;
  step_out(S, B.out_h.p, nsub);
  S.E = (uint32_t)E; S.dim = q_dev ? dim : 0; S.nsub = nsub; S.np = (uint32_t)g->P;
  S.token = next_token(g->step_token);
  step_read_window(S, g->pf_off, g->pf_len, E);
  S.rows_partial = host_rows_partial(c, g->rows_partial);
  nreal = 0;
  for (auto& x : g->subs) nreal += x.kind == SUB_REAL;
  shape = pmk::StepShape{};
  shape.np = (uint32_t)g->P; shape.nsub = nsub; shape.maxPH = g->maxPH; shape.maxSS = g->maxSS; shape.E = (uint32_t)E; shape.ph8 = g->ph8;
  for (uint64_t p = 0; p < g->P; ++p) {
    const uint32_t n = g->sb[p + 1] - g->sb[p];
    shape.max_per_part = std::max(shape.max_per_part, n);
    shape.np_live += n > 0;
  }
  shape.of_caller(pmk::STEP_ENGINE, S.recg && S.err_h);
  shape.unfused = c->no_fuse || c->debug_sync; shape.no_split = c->no_split; shape.no_guess = c->no_guess;
  if (shape.args_valid) {
    memcpy(S.subs_a, g->subs.data(), dsub);
    memcpy(S.sb_a, g->sb.data(), (g->P + 1) * 4);
  }
  ans_bytes = 0;
  for (auto& x : g->subs)
    if (x.kind == SUB_REAL || x.kind == SUB_DUMMY) ans_bytes += answer_bytes(g->parts[x.part].d, E);
  return 0;
}

int engine_step(Engine* g, const float* q_dev, uint32_t dim) {
  auto t_begin = Clock::now();
  pm_ctx* c = g->ctx;
  hipStream_t st = c->stream;
  const uint32_t nsub = (uint32_t)g->subs.size();
  if (nsub == 0) return 0;
  PmStep S;
  pmk::StepShape shape;
  uint32_t nreal;
  double ans_bytes;
  CHK(step_setup(g, q_dev, dim, S, shape, nreal, ans_bytes));
  StepBufs& B = g->buf;
  // One launch (k_step) when the step fits it, else the three kernels (pmk::step_plan).
  std::function<int()> dump_res;
  if (c->debug_sync) dump_res = [&]() -> int {   // validate every resolution record before k_answer consumes it
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
    return 0;
  };
  CHK(step_chain(c, B, S, shape, nreal, ans_bytes, dump_res));
  g->step_seq = c->record_done(st);
  HIPCHK(hipGetLastError());
  c->host_add(HT_STEP_LAUNCH, ms_since(t_begin));
  CHK(wait_and_post(g, S, nsub, t_begin));
  if (S.err_h && *(volatile uint32_t*)S.err_h) {   // only k_step sets it
    *(volatile uint32_t*)S.err_h = 0;
    return fail(PM_EHIP, "k_step: a hand-off wait timed out (results of this step are invalid)");
  }
  return 0;
}
}  // namespace pmh

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
namespace pmh {
void print_stamps(const Engine& e) {
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
}  // namespace pmh
struct pm_pir { Engine e; ~pm_pir() { print_stamps(e); } };

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
namespace pmh {
void record_stats(Engine* g, double t) {   // RecordStats batch-pir.go:110-117
  g->prepTime = t;
  double s = 0; for (auto& p : g->parts) s += part_storage(p, g->Ebytes);
  g->storage = (double)(uint64_t)s;
  double on = 0; for (auto& p : g->parts) on += part_comm(p, g->E) * 2.0;
  g->commOn = (double)(uint64_t)on;
  g->Support = g->parts[0].maxq64 / 2;
  double dbBytes = (double)g->N * (double)g->Ebytes;
  g->commOff = (double)(uint64_t)(dbBytes / (double)g->Support);
}
}  // namespace pmh
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
  CHK(db_guard(&server->e));
  const Engine& s = server->e;
  pm_batchpir* h = new pm_batchpir();
  int r = engine_create(ctx, &h->e, s.N, s.Ebytes, s.B, nullptr, s.F, seed, true, s.shard, s.nshards, &s);
  if (r) { delete h; return r; }
  h->e.pf_off = s.pf_off; h->e.pf_len = s.pf_len;
  *out = h;
  return 0;
}
// A client with no DB on the device: engine_create's parameters, keys and hint tables,
// filled by streamed preprocessings (pm_stream.cpp).
extern "C" int pm_batchpir_create_remote(pm_ctx* ctx, uint64_t DBSize, uint64_t DBEntryByteNum, uint64_t BatchSize,
                                         uint64_t F, uint64_t seed, pm_batchpir** out) {
  if (!out) return fail(PM_EINVAL, "out is NULL");
  if (!ctx) return fail(PM_EINVAL, "ctx is NULL");
  if (DBSize == 0) return fail(PM_EINVAL, "DBSize must be > 0");
  if (DBEntryByteNum < 8) return fail(PM_EINVAL, "DBEntryByteNum must be >= 8");
  if (BatchSize < 2) return fail(PM_EINVAL, "BatchSize must be >= 2");
  pm_batchpir* h = new pm_batchpir();
  int r = engine_create(ctx, &h->e, DBSize, DBEntryByteNum, BatchSize, nullptr, F, seed, true, 0, 1, nullptr, nullptr, 0,
                        true);
  if (r) { delete h; return r; }
  *out = h;
  return 0;
}
extern "C" void pm_batchpir_destroy(pm_batchpir* h) { delete h; }
namespace pmh {
int client_guard(const Engine* g) {
  if (g->pstream.open) return fail(PM_EINVAL, "a streamed preprocessing is open");
  return g->split.open ? fail(PM_EINVAL, "a split query is open") : 0;
}
int db_guard(const Engine* g) {
  return g->remote ? fail(PM_EINVAL, "no DB on this handle") : 0;
}
int batch_prep(Engine* g) {   // Preprocessing (batch-pir.go:119-155)
  CHK(db_guard(g));
  g->pstream.open = false;   // ... and an open stream has nothing left to fill
  g->split.open = false;   // every hint is rebuilt: an open split query (pm_batchpir_client_begin) has nothing left to finish
  g->FBN = 0; g->QMIP = 0;
  auto t0 = std::chrono::steady_clock::now();
  CHK(engine_prep(g, 0, g->P));
  double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  g->prepCount++;
  record_stats(g, t);
  return 0;
}
}  // namespace pmh
extern "C" int pm_batchpir_preprocessing(pm_batchpir* h) { return batch_prep(&h->e); }
extern "C" int pm_batchpir_dummy_preprocessing(pm_batchpir* h) {   // batch-pir.go:157-166
  CHK(client_guard(&h->e));
  h->e.skipPrep = true;
  CHK(engine_prep(&h->e, 0, h->e.P));   // (reads no DB: zero hints)
  h->e.prepared = true;
  record_stats(&h->e, 0);
  return 0;
}

namespace pmh {
// Query (batch-pir.go:170-248).  Partitions whose FinishedQueryNum cannot reach
// MaxQueryNum inside this batch run as fused steps (at most
// step_max_sub_per_part() sub-queries per partition per step); the rest replay
// the reference's per-sub-query re-preprocessing check (pir.go:527-530) one
// sub-query at a time.  q_dev / dist_out: optional L2 of every answer to q.
// Query (batch-pir.go:170-248).  Responses go to out[n][E], or, when rows_out
// is given, rows_out[i] points at response i (pinned result rows of the step,
// the collected rows of a multi-step query, or a zero row); valid until the
// next query on this engine.
int batch_query(Engine* g, const uint64_t* idx, uint64_t n, uint64_t* out, const float* q_dev,
                       uint32_t dim, float* dist_out, const uint64_t** rows_out,
                       uint8_t* ok) {
  CHK(db_guard(g));
  CHK(client_guard(g));
  auto t = Clock::now();
  int r = batch_query_impl(g, idx, n, out, q_dev, dim, dist_out, rows_out, ok);
  g->ctx->host_add(HT_BATCH_QUERY, ms_since(t));
  return r;
}
}  // namespace pmh
static inline bool status_ok(uint32_t st) { return st == ST_OK || st == ST_CACHED || st == ST_DUP; }

namespace pmh {
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
int bq_prepare(Engine* g, const uint64_t* idx, uint64_t n, bool* fast) {
  CHK(client_guard(g));   // (the entry points check first, before they change anything)
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
void bq_emit_fast(Engine* g, const uint64_t* idx, uint64_t n, uint64_t* out, float* dist_out,
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
int bq_tail(Engine* g, uint64_t n) {
  if (g->QMIP >= g->parts[0].maxq64 - 2) {
    if (g->remote) g->prep_due = true;   // no DB to preprocess over: the caller streams it (pm_batchpir_prep_due)
    else CHK(batch_prep(g));
  } else {
    g->FBN += n / g->B;
    g->QMIP += g->qn;
  }
  return 0;
}
int batch_query_impl(Engine* g, const uint64_t* idx, uint64_t n, uint64_t* out, const float* q_dev,
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
}  // namespace pmh
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
  CHK(db_guard(g));
  CHK(client_guard(g));
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
extern "C" int pm_batchpir_step_spec(pm_batchpir* h, uint32_t* out, uint64_t cap, uint64_t* nsub) {
  if (!h || !nsub || (!out && cap)) return fail(PM_EINVAL, "NULL argument");
  Engine& g = h->e;
  if (!g.ctx->step_spec) return fail(PM_EINVAL, "no speculation record: the context was created without PM_STEP_SPEC=1");
  const uint32_t n = g.buf.spec_nsub;
  if (!n) return fail(PM_EINVAL, "no speculation record: the last step did not run k_step");
  *nsub = n;
  if (!out) return 0;   // the count alone
  if (cap < n) return fail(PM_EINVAL, "out holds fewer words than the step has sub-queries");
  HIPCHK(hipSetDevice(g.ctx->device));
  HIPCHK(hipStreamSynchronize(g.ctx->stream));
  HIPCHK(hipMemcpy(out, g.buf.specrec.p, (size_t)n * 4, hipMemcpyDeviceToHost));
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
extern "C" uint64_t pm_batchpir_max_set_size(pm_batchpir* h) {
  uint64_t m = 0;
  if (h) for (const PartHost& p : h->e.parts) m = std::max<uint64_t>(m, p.d.SS);
  return m;
}
// The server role: PianoPIRServer.PrivateQuery (pir.go:65-88)
// of nq client-supplied offset sets, each over the partition it names.  Reads
// the handle's DB (or its packed row image) and nothing of the client.
extern "C" int pm_batchpir_server_answer(pm_batchpir* h, const uint32_t* parts, const uint32_t* offsets,
                                         uint64_t stride, uint64_t nq, uint64_t* out) {
  constexpr uint64_t kChunk = 65536;   // sets per upload / launch / download
  if (nq == 0) return 0;
  if (!h || !parts || !offsets || !out) return fail(PM_EINVAL, "NULL argument");
  Engine* g = &h->e;
  pm_ctx* c = g->ctx;
  const uint64_t E = g->E;
  CHK(db_guard(g));
  if (stride < pm_batchpir_max_set_size(h)) return fail(PM_EINVAL, "stride must be >= the largest SetSize");
  if (stride >> 32) return fail(PM_EINVAL, "stride must be < 2^32");
  // every set is checked before any HIP call; the rows each chunk gathers are counted on the way
  std::vector<uint64_t> gathered((nq + kChunk - 1) / kChunk, 0);
  for (uint64_t s = 0; s < nq; ++s) {
    const uint64_t p = parts[s];
    if (p >= g->P) return fail(PM_EINVAL, "partition out of range: set " + std::to_string(s));
    if (!g->parts[p].owned) return fail(PM_EINVAL, "partition not on this shard: set " + std::to_string(s));
    const PmPart& d = g->parts[p].d;
    const uint32_t* o = offsets + s * stride;
    uint64_t rows = 0;
    for (uint64_t i = 0; i < d.SS; ++i) {
      if (o[i] >= d.CS) return fail(PM_EINVAL, "offset out of range: set " + std::to_string(s) + ", chunk " + std::to_string(i));
      rows += i * d.CS + o[i] < d.N;
    }
    gathered[s / kChunk] += rows;
  }
  HIPCHK(hipSetDevice(c->device));
  if (!g->srv_parts_up) {
    std::vector<PmSrvPart> v(g->P);
    for (uint64_t p = 0; p < g->P; ++p) {
      const PmPart& d = g->parts[p].d;
      v[p] = PmSrvPart{d.N, d.row0, d.CS, d.SS};
    }
    CHK(g->srv_parts.reserve(g->P * sizeof(PmSrvPart)));
    HIPCHK(hipMemcpy(g->srv_parts.p, v.data(), g->P * sizeof(PmSrvPart), hipMemcpyHostToDevice));
    g->srv_parts_up = true;
  }
  const uint64_t cap = std::min(nq, kChunk);
  CHK(g->qoffs.reserve(cap * stride * 4 + cap * 4));   // the chunk's sets, then their partitions
  CHK(g->ans_srv.reserve(cap * E * 8));
  const uint64_t* const dbp = g->apk_nseg ? g->apk->as<uint64_t>() : nullptr;
  const double row_bytes = dbp ? g->apk_nseg * 16.0 : (double)(E & ~3ull) * 8;
  for (uint64_t s0 = 0; s0 < nq; s0 += kChunk) {
    const uint64_t n = std::min(kChunk, nq - s0);
    uint32_t* const qpart = g->qoffs.as<uint32_t>() + cap * stride;
    HIPCHK(hipMemcpyAsync(g->qoffs.p, offsets + s0 * stride, n * stride * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(qpart, parts + s0, n * 4, hipMemcpyHostToDevice, c->stream));
    c->timed("server_answer", (double)gathered[s0 / kChunk] * row_bytes, [&] {
      pmk::server_answer_parts(c->stream, g->srv_parts.as<PmSrvPart>(), qpart, g->qoffs.as<uint32_t>(), (uint32_t)n,
                               (uint32_t)stride, g->db->as<uint64_t>(), dbp, g->apk_nseg, g->apk_cseg, (uint32_t)E,
                               g->ans_srv.as<uint64_t>());
    });
    HIPCHK(hipGetLastError());
    if (dbp) c->host_add(HT_SERVER_ANSWER_PACKED, 0.0);
    HIPCHK(hipMemcpyAsync(out + s0 * E, g->ans_srv.p, n * E * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return 0;
}
// The client role: SimpleBatchPianoPIR.Query cut at the wire.
// begin is Query up to server.PrivateQuery (bucketing, the step's hint search
// and resolution, the sets out); finish is the rest of it over the server's
// answers (the answer kernels' epilogue, the host mirrors, the responses, the
// batch counters and trigger).
extern "C" uint64_t pm_batchpir_client_max_sets(pm_batchpir* h, uint64_t n) {
  return h ? h->e.P * (n / h->e.P) : 0;
}
extern "C" int pm_batchpir_client_begin(pm_batchpir* h, const uint64_t* ids, uint64_t n, uint32_t* parts,
                                        uint32_t* offsets, uint64_t stride, uint64_t cap, uint64_t* nq) {
  if (!h || !ids || !parts || !offsets || !nq) return fail(PM_EINVAL, "NULL argument");
  Engine* g = &h->e;
  pm_ctx* c = g->ctx;
  const uint64_t E = g->E, P = g->P, qn = n / P;
  CHK(client_guard(g));
  if (g->remote && !g->prepared) return fail(PM_EINVAL, "not preprocessed");
  if (g->prep_due) return fail(PM_EINVAL, "preprocessing due: stream it first");
  if (g->nshards > 1) return fail(PM_EINVAL, "the client role is not built for shard handles");
  if (E > pmk::client_max_e() || g->maxSS > pmk::client_max_ss())
    return fail(PM_EINVAL, "the client role serves DBEntrySize <= 256 words and SetSize <= 1024");
  for (uint64_t i = 0; i < n; ++i)
    if (ids[i] >= g->N) return fail(PM_EINVAL, "id " + std::to_string(ids[i]) + " >= DBSize");
  if (stride < g->maxSS) return fail(PM_EINVAL, "stride must be >= the largest SetSize");
  if (qn == 0 || qn > pmk::step_max_sub_per_part())
    return fail(PM_EINVAL, "n / PartitionNum must be in [1, " + std::to_string(pmk::step_max_sub_per_part()) + "]");
  if (cap < P * qn) return fail(PM_EINVAL, "cap must be >= pm_batchpir_client_max_sets");
  auto t_begin = Clock::now();
  {   // bq_prepare's budget rule, before anything moves: the first qn ids of a partition are its sub-queries
    std::vector<uint64_t> cnt(P, 0);
    for (uint64_t i = 0; i < n; ++i) ++cnt[g->part_of(ids[i])];
    for (uint64_t p = 0; p < P; ++p)
      if (g->parts[p].fqn + std::min(cnt[p], qn) >= g->parts[p].maxq64)
        return fail(PM_EINVAL, "partition at its query budget: preprocess first");
  }
  // every buffer of the call is reserved before the bucketing moves anything (the dummy counters): the step has
  // P * qn sub-queries, as every partition is this handle's
  Engine::SplitQuery& Q = g->split;
  const uint32_t qw = (g->maxSS + 3) & ~3u;
  const size_t set_bytes = (size_t)P * qn * qw * 4, down = set_bytes + (size_t)P * qn * 4;
  HIPCHK(hipSetDevice(c->device));
  CHK(Q.sets_d.reserve(down));
  CHK(Q.sets_h.reserve(down));
  CHK(g->buf.reserve((uint32_t)(P * qn), (uint32_t)P, (g->maxPH + 63) / 64, pmk::step_match_blocks(g->maxPH), E));
  CHK(g->buf.desc_h.reserve(P * qn * sizeof(PmSub) + (P + 1) * 4));
  CHK(g->buf.out_h.reserve(step_out_bytes((uint32_t)(P * qn), E)));
  bool fast = false;
  CHK(bq_prepare(g, ids, n, &fast));
  const uint32_t nsub = (uint32_t)g->subs.size();
  if (!fast || nsub != P * qn) return fail(PM_EINVAL, "the batch does not fit one step");   // (excluded by the checks above)
  PmStep& S = Q.S;
  pmk::StepShape shape;
  uint32_t nreal;
  double ans_bytes;
  CHK(step_setup(g, nullptr, 0, S, shape, nreal, ans_bytes));
  shape.unfused = true;   // the hint search and the resolution as launches of their own, whatever the context says
  shape.no_split = true;
  uint32_t* const modes_d = Q.sets_d.as<uint32_t>() + (size_t)nsub * qw;
  CHK(step_chain(c, g->buf, S, shape, nreal, 0, [&]() -> int {
    c->timed("client_sets", (double)down, [&] { pmk::client_sets(c->stream, S, Q.sets_d.as<uint32_t>(), modes_d, qw); });
    return kChainStop;
  }));
  HIPCHK(hipGetLastError());
  // from here on the hints have moved: the query is open whatever happens to the copy
  Q.open = true;
  Q.ids.assign(ids, ids + n);
  Q.map.assign(nsub, ~0u);
  Q.nq = 0;
  HIPCHK(hipMemcpyAsync(Q.sets_h.p, Q.sets_d.p, down, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  // the sending rows, compacted on the way out
  const uint32_t* const sets = Q.sets_h.as<uint32_t>();
  const uint32_t* const modes = sets + (size_t)nsub * qw;
  uint64_t k = 0;
  for (uint32_t s = 0; s < nsub; ++s) {
    if (!pmk::client_mode_sends(modes[s])) continue;
    const uint32_t SS = g->parts[g->subs[s].part].d.SS;
    uint32_t* o = offsets + k * stride;
    memcpy(o, sets + (size_t)s * qw, (size_t)SS * 4);
    memset(o + SS, 0, (size_t)(stride - SS) * 4);
    parts[k] = g->subs[s].part;
    if (pmk::client_mode_reads(modes[s])) Q.map[s] = (uint32_t)k;
    ++k;
  }
  Q.nq = k;
  *nq = k;
  c->host_add(HT_CLIENT_BEGIN, ms_since(t_begin));
  return 0;
}
extern "C" int pm_batchpir_client_finish(pm_batchpir* h, const uint64_t* answers, uint64_t nq, uint64_t* out,
                                         uint8_t* ok) {
  if (!h || !out || (!answers && nq)) return fail(PM_EINVAL, "NULL argument");
  Engine* g = &h->e;
  pm_ctx* c = g->ctx;
  Engine::SplitQuery& Q = g->split;
  if (g->pstream.open) return fail(PM_EINVAL, "a streamed preprocessing is open");
  if (!Q.open) return fail(PM_EINVAL, "no split query is open");
  if (nq != Q.nq) return fail(PM_EINVAL, "nq is not the number of sets pm_batchpir_client_begin returned");
  auto t_begin = Clock::now();
  const uint64_t E = g->E, n = Q.ids.size();
  const PmStep& S = Q.S;
  const uint32_t nsub = S.nsub;
  HIPCHK(hipSetDevice(c->device));
  CHK(Q.ans_d.reserve(std::max<uint64_t>(1, nq) * E * 8));
  CHK(Q.map_d.reserve((size_t)nsub * 4));
  Q.open = false;   // no abort: a failure below leaves nothing to finish either
  if (nq) HIPCHK(hipMemcpyAsync(Q.ans_d.p, answers, nq * E * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(Q.map_d.p, Q.map.data(), (size_t)nsub * 4, hipMemcpyHostToDevice, c->stream));
  c->timed("client_finish", (double)nq * E * 8,
           [&] { pmk::client_finish(c->stream, S, Q.ans_d.as<uint64_t>(), Q.map_d.as<uint32_t>()); });
  g->step_seq = c->record_done(c->stream);
  HIPCHK(hipGetLastError());
  CHK(wait_and_post(g, S, nsub, t_begin));
  bq_emit_fast(g, Q.ids.data(), n, out, nullptr, nullptr, ok);
  c->host_add(HT_CLIENT_FINISH, ms_since(t_begin));
  return bq_tail(g, n);
}
extern "C" int pm_batchpir_export(pm_batchpir* h, uint64_t p, uint32_t* rk, uint64_t* pt, uint64_t* par,
                                  uint64_t* pp, uint64_t* bt, uint64_t* bpar, uint64_t* ri, uint64_t* rv,
                                  uint64_t* hist) {
  if (p >= h->e.P || !h->e.parts[p].owned) return fail(PM_EINVAL, "partition not held by this shard");
  return engine_export(&h->e, p, rk, pt, par, pp, bt, bpar, ri, rv, hist);
}
