// pm_stream.cpp — the streamed hint preprocessing of a batch PIR client
// (pm_batchpir_prep_stream_*): Piano's offline protocol, in
// which the DB passes the client once, chunk by chunk, and is never stored
// (PianoPIRClient.UpdatePreprocessing, pir.go:303-352), and the server's side
// of that stream (pm_batchpir_server_rows).  Needs pm_ctx.cpp and pm_engine.cpp.
#include "pm_engine.h"

namespace pmh {
std::atomic<int> g_stream_upload_only{0};
}

static constexpr uint64_t kStreamWindowBytes = 8ull << 20;

// rows [*lo, *lo + n) of partition d that exist in chunks [c0, c0 + nc); returns n
static uint64_t window_rows(const PmPart& d, uint64_t c0, uint64_t nc, uint64_t* lo) {
  *lo = c0 * d.CS;
  const uint64_t hi = std::min<uint64_t>((c0 + nc) * d.CS, d.N);
  return hi > *lo ? hi - *lo : 0;
}

// Client.Initialization of every partition (engine_prep_host + prep_init +
// prep_offsets: the next epoch's key, tags, program points, histogram, PRF
// tables), zero parities and replacement values, and an open stream.
extern "C" int pm_batchpir_prep_stream_begin(pm_batchpir* h) {
  if (!h) return fail(PM_EINVAL, "NULL argument");
  Engine* g = &h->e;
  pm_ctx* c = g->ctx;
  if (g->nshards > 1) return fail(PM_EINVAL, "the streamed preprocessing is not built for shard handles");
  Engine::PrepStream& ps = g->pstream;
  HIPCHK(hipSetDevice(c->device));
  // the staging slots, sized once and before anything moves: a sub-window of the largest chunk, or 8 MiB
  // (less where no partition has that many bytes)
  uint64_t part_bytes = 0;
  for (const PartHost& p : g->parts) part_bytes = std::max<uint64_t>(part_bytes, (uint64_t)p.d.SS * p.d.CS * g->Ebytes);
  const uint64_t slot = std::min(part_bytes, std::max<uint64_t>(kStreamWindowBytes, (uint64_t)g->maxCS * g->Ebytes));
  for (int i = 0; i < 2; ++i) {
    CHK(ps.stage[i].reserve(slot));
    CHK(ps.win[i].reserve(slot));
    if (!ps.ev[i]) HIPCHK(hipEventCreateWithFlags(&ps.ev[i], hipEventDisableTiming));
  }
  ps.slot_bytes = slot;
  // an open stream is abandoned (its epoch is spent), an open split query has nothing left to finish
  ps.open = false;
  g->split.open = false;
  std::vector<uint64_t> todo;
  CHK(engine_prep_host(g, 0, g->P, todo));   // synchronises the stream: an abandoned stream's windows have left the slots
  ps.busy[0] = ps.busy[1] = false;
  ps.next = 0;
  hipStream_t st = c->stream;
  const PmPart* dp = g->owned_d.as<PmPart>();
  const int np = (int)todo.size();
  double aes = 0;
  for (uint64_t i : todo) aes += (double)g->parts[i].d.H * g->parts[i].d.SS;
  c->timed("prep_init", 0, [&] { pmk::prep_init(st, dp, np, g->maxH, g->maxRepl, (uint32_t)g->E, false); });
  c->timed("prep_offsets", aes, [&] { pmk::prep_offsets(st, dp, np, g->maxH, g->maxSS); });
  HIPCHK(hipMemsetAsync(g->parity.p, 0, g->parity.n, st));
  HIPCHK(hipMemsetAsync(g->rval.p, 0, g->rval.n, st));
  HIPCHK(hipGetLastError());
  ps.got.assign(g->P, {});
  ps.missing = 0;
  for (uint64_t p = 0; p < g->P; ++p) {
    ps.got[p].assign(g->parts[p].d.SS, 0);
    ps.missing += g->parts[p].d.SS;
  }
  ps.t0 = Clock::now();
  ps.open = true;
  return 0;
}

// UpdatePreprocessing of chunks [chunk0, chunk0 + nchunks) of one partition.
// The caller's rows go through the two staging slots in sub-windows of whole
// chunks; nothing here waits for the stream except for a slot's previous use,
// so the upload of one sub-window overlaps the fold of the one before.
extern "C" int pm_batchpir_prep_stream_rows(pm_batchpir* h, uint32_t partition, uint32_t chunk0, uint32_t nchunks,
                                            const uint64_t* rows, uint64_t nrows) {
  if (!h) return fail(PM_EINVAL, "NULL argument");
  Engine* g = &h->e;
  pm_ctx* c = g->ctx;
  Engine::PrepStream& ps = g->pstream;
  if (!ps.open) return fail(PM_EINVAL, "no streamed preprocessing is open");
  if (partition >= g->P) return fail(PM_EINVAL, "partition out of range");
  const PmPart& d = g->parts[partition].d;
  if (nchunks == 0) return fail(PM_EINVAL, "nchunks must be > 0");
  if ((uint64_t)chunk0 + nchunks > d.SS) return fail(PM_EINVAL, "chunk0 + nchunks must be <= SetSize");
  uint64_t lo;
  const uint64_t want = window_rows(d, chunk0, nchunks, &lo);
  if (nrows != want)
    return fail(PM_EINVAL, "nrows must be " + std::to_string(want) + ", the existing rows of these chunks");
  if (!rows && nrows) return fail(PM_EINVAL, "rows is NULL");
  std::vector<char>& got = ps.got[partition];
  for (uint32_t k = chunk0; k < chunk0 + nchunks; ++k)
    if (got[k]) return fail(PM_EINVAL, "chunk already delivered: partition " + std::to_string(partition) + ", chunk " + std::to_string(k));
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const uint64_t E = g->E, chunk_bytes = (uint64_t)d.CS * g->Ebytes;
  const uint32_t per = (uint32_t)std::max<uint64_t>(1, ps.slot_bytes / chunk_bytes);   // chunks per sub-window
  const bool upload_only = g_stream_upload_only.load() != 0;
  const PmPart* dparts = g->parts_d.as<PmPart>();
  for (uint32_t c0 = chunk0; c0 < chunk0 + nchunks; c0 += per) {
    const uint32_t nc = std::min(per, chunk0 + nchunks - c0);
    uint64_t wlo;
    const uint64_t nr = window_rows(d, c0, nc, &wlo);
    const uint32_t s = ps.next;
    ps.next ^= 1u;
    if (ps.busy[s]) HIPCHK(hipEventSynchronize(ps.ev[s]));   // the slot's last window has been folded
    uint64_t* const win = ps.win[s].as<uint64_t>();
    if (nr) {
      memcpy(ps.stage[s].p, rows + (wlo - lo) * E, nr * E * 8);
      HIPCHK(hipMemcpyAsync(win, ps.stage[s].p, nr * E * 8, hipMemcpyHostToDevice, st));
    }
    if (!g->skipPrep && !upload_only) {   // (DummyPreprocessing leaves the engine with zero hints, streamed or not)
      // the fold's algorithmic bytes as engine_prep_launch counts them: every chunk is selected by all
      // hints but the backups of its own group
      const double fold = ((double)d.PH + (double)(d.SS - 1) * d.Qpc) * nc * (double)E * 8;
      c->timed("prep_stream_fold", fold,
               [&] { pmk::stream_fold(st, dparts, partition, d.H, win, c0, nc, (uint32_t)nr, (uint32_t)E); });
      c->timed("prep_stream_repl", (double)nc * d.Qpc * E * 8 * 2,
               [&] { pmk::stream_repl(st, dparts, partition, d.Qpc, win, c0, nc, (uint32_t)nr, (uint32_t)E); });
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ps.ev[s], st));
    ps.busy[s] = true;
    for (uint32_t k = c0; k < c0 + nc; ++k) got[k] = 1;
    ps.missing -= nc;
    c->host_add(HT_PREP_STREAM_WINDOWS, 0.0);
  }
  return 0;
}

// The rest of batch_prep after its preprocessing: the batch counters, PrepCount
// and the statistics; the handle then equals one that ran pm_batchpir_preprocessing.
extern "C" int pm_batchpir_prep_stream_end(pm_batchpir* h) {
  if (!h) return fail(PM_EINVAL, "NULL argument");
  Engine* g = &h->e;
  pm_ctx* c = g->ctx;
  Engine::PrepStream& ps = g->pstream;
  if (!ps.open) return fail(PM_EINVAL, "no streamed preprocessing is open");
  if (ps.missing)
    for (uint64_t p = 0; p < g->P; ++p)
      for (uint32_t k = 0; k < ps.got[p].size(); ++k)
        if (!ps.got[p][k])
          return fail(PM_EINVAL, "chunks missing: partition " + std::to_string(p) + ", chunk " + std::to_string(k));
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipGetLastError());
  ps.open = false;
  ps.busy[0] = ps.busy[1] = false;
  const double ms = ms_since(ps.t0);
  g->FBN = 0; g->QMIP = 0;
  g->prepCount++;
  record_stats(g, ms / 1e3);
  g->prep_due = false;
  g->prepared = true;
  c->host_add(HT_PREP_STREAM, ms);
  return 0;
}

extern "C" int pm_batchpir_prep_due(pm_batchpir* h) { return h && h->e.prep_due ? 1 : 0; }

// The server's side of the stream: the existing rows of chunks [chunk0, chunk0 +
// nchunks) of one partition, device to host.  Reads the DB only.
extern "C" int pm_batchpir_server_rows(pm_batchpir* h, uint32_t partition, uint32_t chunk0, uint32_t nchunks,
                                       uint64_t* rows, uint64_t cap_rows, uint64_t* nrows) {
  if (!h || !nrows) return fail(PM_EINVAL, "NULL argument");
  Engine* g = &h->e;
  CHK(db_guard(g));
  if (partition >= g->P) return fail(PM_EINVAL, "partition out of range");
  if (!g->parts[partition].owned) return fail(PM_EINVAL, "partition not on this shard");
  const PmPart& d = g->parts[partition].d;
  if (nchunks == 0) return fail(PM_EINVAL, "nchunks must be > 0");
  if ((uint64_t)chunk0 + nchunks > d.SS) return fail(PM_EINVAL, "chunk0 + nchunks must be <= SetSize");
  uint64_t lo;
  const uint64_t n = window_rows(d, chunk0, nchunks, &lo);
  *nrows = n;
  if (cap_rows < n) return fail(PM_EINVAL, "cap_rows is below the rows of these chunks (*nrows)");
  if (n == 0) return 0;
  if (!rows) return fail(PM_EINVAL, "rows is NULL");
  HIPCHK(hipSetDevice(g->ctx->device));
  HIPCHK(hipMemcpy(rows, g->db->as<uint64_t>() + (d.row0 + lo) * g->E, n * g->E * 8, hipMemcpyDeviceToHost));
  return 0;
}
