// pm_ctx.cpp — the bottom layer of the host side: the error text behind
// pm_last_error, the AES key schedule, the context with its kernel timing,
// pm_set_option and the option words it sets, and the leaf batches.
#include "pm_host.h"

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local std::string g_err;
namespace pmh {
int fail(int code, const std::string& msg) { g_err = msg; return code; }
}  // namespace pmh

extern "C" const char* pm_last_error(void) { return g_err.c_str(); }

// ---------------------------------------------------------------------------
// host AES-128 key schedule (FIPS-197 §5.2; expandKeyAsm, aes_amd64.s:87-126)
// ---------------------------------------------------------------------------
static constexpr AesTables kAes{};
extern "C" int pm_expand_key(const uint8_t key[16], uint32_t rk[44]) {
  uint8_t w[176];
  memcpy(w, key, 16);
  uint8_t rcon = 1;
  for (int i = 16; i < 176; i += 4) {
    uint8_t t[4] = {w[i - 4], w[i - 3], w[i - 2], w[i - 1]};
    if (i % 16 == 0) {
      uint8_t u = t[0];
      t[0] = kAes.sbox[t[1]] ^ rcon; t[1] = kAes.sbox[t[2]]; t[2] = kAes.sbox[t[3]]; t[3] = kAes.sbox[u];
      rcon = AesTables::gmul(rcon, 2);
    }
    for (int k = 0; k < 4; ++k) w[i + k] = w[i - 16 + k] ^ t[k];
  }
  memcpy(rk, w, 176);   // little-endian word view, as the GPU and AESENC read it
  return 0;
}


extern "C" int pm_ctx_create(int device, pm_ctx** out) {
  if (!out) return fail(PM_EINVAL, "out is NULL");
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(PM_EINVAL, "no such HIP device " + std::to_string(device));
  HIPCHK(hipSetDevice(device));
  // Each online step ends in one host wait; spin instead of yielding so the
  // host resumes the beam search as soon as the GPU finishes.  Ignored if the
  // device is already initialised with other flags.
  (void)hipSetDeviceFlags(hipDeviceScheduleSpin);
  (void)hipGetLastError();
  pm_ctx* c = new pm_ctx();
  c->device = device;
  const char* dbg = getenv("PM_DEBUG_SYNC");
  c->debug_sync = dbg && dbg[0] == '1';
  const char* nf = getenv("PM_NO_FUSE");
  c->no_fuse = nf && nf[0] == '1';
  const char* ns = getenv("PM_NO_SPLIT");
  c->no_split = ns && ns[0] == '1';
  const char* ls = getenv("PM_LOG_STEPS");
  c->log_steps = ls && ls[0] == '1';
  const char* dc = getenv("PM_DEBUG_CACHE");
  c->debug_cache = dc && dc[0] == '1';
  const char* vr = getenv("PM_VERIFY_ROWS");
  c->verify_rows = vr && vr[0] == '1';
  if (const char* rc = getenv("PM_ROWS_CHECK")) c->rows_check = atoi(rc);
  c->hash_mult.resize(pmk::step_max_e());
  for (size_t w = 0; w < c->hash_mult.size(); ++w) c->hash_mult[w] = row_hash_mult(w);
  if (const char* pw = getenv("PM_PUBLISH_WAIT")) c->publish_wait = pw[0] != '0';
  if (c->publish_wait) {
    for (auto& e : c->done_ring)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventReleaseToSystem) != hipSuccess) {
        delete c;
        return fail(PM_EHIP, "hipEventCreateWithFlags(step completion) failed");
      }
    c->done_ev = c->done_ring[0];
  }
  if (const char* rs = getenv("PM_REPL_SIDE")) c->repl_side = rs[0] != '0';
  const char* ng = getenv("PM_NO_GUESS");
  c->no_guess = ng && ng[0] == '1';
  const char* sr = getenv("PM_STEP_SPEC");
  c->step_spec = sr && sr[0] == '1';
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) { delete c; return fail(PM_EHIP, hipGetErrorString(e)); }
  *out = c;
  return 0;
}
extern "C" void pm_ctx_destroy(pm_ctx* c) { if (c) { (void)hipSetDevice(c->device); delete c; } }
extern "C" int pm_ctx_sync(pm_ctx* c) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipGetLastError()); return 0; }
extern "C" int pm_ctx_mem_info(pm_ctx* c, uint64_t* free_b, uint64_t* total_b) {
  if (!c) return fail(PM_EINVAL, "ctx is NULL");
  HIPCHK(hipSetDevice(c->device));
  size_t f = 0, t = 0;
  HIPCHK(hipMemGetInfo(&f, &t));
  if (free_b) *free_b = f;
  if (total_b) *total_b = t;
  return 0;
}
// Timeline base: one event recorded when kernel timing is first enabled in the
// process; every timed launch's start / end can then be placed on one time axis
// (hipEventElapsedTime between events of one device, any streams).
static std::mutex g_tl_mu;
static hipEvent_t g_tl_base = nullptr;
extern "C" int pm_timing_enable(pm_ctx* c, int on) {
  c->timing = on;
  if (on >= 2) {
    std::lock_guard<std::mutex> lk(g_tl_mu);
    if (!g_tl_base) {
      HIPCHK(hipEventCreate(&g_tl_base));
      HIPCHK(hipEventRecord(g_tl_base, c->stream));
    }
  }
  return 0;
}
// Diagnostics: append "name,start_us,end_us,ctx" for every timed launch of c
// (relative to the process's timeline base) to `path`.
extern "C" int pm_timing_timeline(pm_ctx* c, const char* path) {
  if (!c || !path) return fail(PM_EINVAL, "NULL argument");
  HIPCHK(hipStreamSynchronize(c->stream));
  std::lock_guard<std::mutex> lk(g_tl_mu);
  if (!g_tl_base) return fail(PM_EINVAL, "no timeline (kernel timing level 2 never enabled)");
  FILE* f = fopen(path, "a");
  if (!f) return fail(PM_EINVAL, std::string("cannot open ") + path);
  for (auto& t : c->launches) {
    float a = 0, b = 0;
    if (hipEventElapsedTime(&a, g_tl_base, t.a) != hipSuccess || hipEventElapsedTime(&b, g_tl_base, t.b) != hipSuccess)
      continue;
    fprintf(f, "%s,%.3f,%.3f,%p\n", t.name.c_str(), a * 1e3, b * 1e3, (void*)c);
  }
  fclose(f);
  return 0;
}
namespace pmh {
// "verify_records" (sharded loop): check the records of every value-th shared
// step of each team on the host (0: off); read when a loop starts
std::atomic<int> g_verify_records{0};
// "device_loop": pm_search_loop_batched's device loop (run_batched_dev) 1 / 0;
// -1: the environment's choice (PM_DEVICE_LOOP, default 1)
std::atomic<int> g_device_loop{-1};
// Bound on the communicators' creation and on the probe (pm_set_option
// "rccl_timeout_s", else PM_RCCL_TIMEOUT_S, default 120 s): a rank whose peer
// never joins returns PM_ETIMEDOUT instead of blocking inside RCCL.
std::atomic<int> g_rccl_timeout_s{-1};
// fault seam (tests): run_batched_dev fails before queueing query n (-1: off)
std::atomic<int> g_fault_drl_query{-1};
}  // namespace pmh
extern "C" int pm_set_option(const char* name, int value) {
  if (!name) return fail(PM_EINVAL, "NULL argument");
  if (!strcmp(name, "verify_records")) { g_verify_records.store(value < 0 ? 0 : value); return 0; }
  if (!strcmp(name, "rccl_timeout_s")) { g_rccl_timeout_s.store(value); return 0; }
  if (!strcmp(name, "device_loop")) { g_device_loop.store(value < 0 ? -1 : value); return 0; }
  if (!strcmp(name, "fault_drl_query")) { g_fault_drl_query.store(value); return 0; }
  if (!strcmp(name, "stream_upload_only")) { g_stream_upload_only.store(value > 0 ? 1 : 0); return 0; }
  if (!strcmp(name, "aes_bs")) { pmk::set_aes_bs(value); return 0; }
  if (!strcmp(name, "fold_rot")) {
    if (value < -1 || value > 1) return fail(PM_EINVAL, "fold_rot takes 1, 0 or -1");
    pmk::set_fold_rot(value);
    return 0;
  }
  if (!strcmp(name, "fold_pack")) {
    if (value < -1 || value > 1) return fail(PM_EINVAL, "fold_pack takes 1, 0 or -1");
    pmk::set_fold_pack(value);
    return 0;
  }
  if (!strcmp(name, "fold_bits")) {
    if (value < -1 || value > 1) return fail(PM_EINVAL, "fold_bits takes 1, 0 or -1");
    pmk::set_fold_bits(value);
    return 0;
  }
  if (!strcmp(name, "answer_pack")) {
    if (value < -1 || value > 1) return fail(PM_EINVAL, "answer_pack takes 1, 0 or -1");
    pmk::set_answer_pack(value);
    return 0;
  }
  if (!strcmp(name, "step_help") && value != -2 && (value < 0 || value > 3))
    return fail(PM_EINVAL, "step_help takes 0..3 or -2");
  if (!strcmp(name, "step_help_spoil") && value != -2 && (value < 0 || value > 7))
    return fail(PM_EINVAL, "step_help_spoil takes a mask 0..7 or -2");
  if (pmk::set_option(name, value)) return fail(PM_EINVAL, std::string("unknown option ") + name);
  return 0;
}
// pmk::step_plan for a shape, as the steps themselves ask it: the caller kind's
// descriptor facts by StepShape::of_caller (an engine always has k_step's
// granules), the options' current values.  Host arithmetic only.
extern "C" int pm_step_plan(const pm_step_shape* in, pm_step_forms* out) {
  if (!in || !out) return fail(PM_EINVAL, "NULL argument");
  if (in->kind > (uint32_t)pmk::STEP_DEVICE || in->nsub == 0 || in->np == 0) return fail(PM_EINVAL, "bad step shape");
  pmk::StepShape s{};
  s.np = in->np; s.nsub = in->nsub; s.np_live = in->np_live; s.max_per_part = in->max_per_part;
  s.maxPH = in->maxPH; s.maxSS = in->maxSS; s.E = in->E; s.ph8 = in->ph8 != 0;
  s.of_caller((int)in->kind, true);
  s.unfused = in->no_fuse != 0; s.no_split = in->no_split != 0; s.no_guess = in->no_guess != 0;
  const pmk::StepPlan p = pmk::step_plan(s, pmk::step_opts());
  static_assert(sizeof out->counter / sizeof out->counter[0] == pmk::STAGE_COUNT, "one slot per launch of a plan");
  *out = pm_step_forms{};
  for (int i = 0; i < pmk::STAGE_COUNT; ++i) {
    const pmk::StepLaunch& l = p.at[i];
    if (l.form < 0) continue;
    out->counter[i] = kHostTimerName[pm_ctx::step_counter(i, l.form)];
    out->grid_x[i] = l.gx; out->grid_y[i] = l.gy; out->block[i] = l.block;
  }
  out->nhelp = p.nhelp; out->nsplit = p.nsplit; out->qw = p.qw; out->np_live = p.np_live; out->cblk = p.cblk;
  out->no_guess = p.no_guess; out->qset = p.qset; out->args_valid = s.args_valid;
  return 0;
}
// pmk::fold_image_map, the map k_fold_image itself evaluates.  Host arithmetic only.
extern "C" int pm_fold_image_map(uint32_t cs, uint32_t ss, uint32_t E, uint32_t dim, int packed, uint64_t x0,
                                 uint64_t n, uint64_t* row, uint32_t* word, uint8_t* is_packed, uint64_t* nitems,
                                 uint32_t* npk_out) {
  if ((n && (!row || !word || !is_packed)) || !nitems || !npk_out) return fail(PM_EINVAL, "NULL argument");
  if ((cs != 512 && cs != 1024) || ss == 0 || ss % 4 || E < 4 || E % 2) return fail(PM_EINVAL, "not a fold image shape");
  const uint32_t npk = packed ? pmk::fold_pack_shape(E, dim) : 0;
  if (packed && (!npk || cs != 512)) return fail(PM_EINVAL, "these entries have no packed fold image");
  *nitems = pmk::fold_image_words(ss, E, cs, npk) / 2;
  *npk_out = npk;
  if (x0 > *nitems || n > *nitems - x0) return fail(PM_EINVAL, "items past the image");
  pmk::fold_image_map(cs, ss, npk, x0, n, row, word, is_packed);
  return 0;
}
extern "C" int pm_timing_reset(pm_ctx* c) {
  HIPCHK(hipStreamSynchronize(c->stream));
  for (auto& t : c->launches) { c->pool.push_back(t.a); c->pool.push_back(t.b); }
  c->launches.clear();
  for (int i = 0; i < HT_COUNT; ++i) { c->host_n[i] = 0; c->host_ms[i] = 0; }
  return 0;
}
extern "C" int pm_timing_get(pm_ctx* c, const char* name, uint64_t* launches, double* total_ms,
                             double* bytes) {
  HIPCHK(hipStreamSynchronize(c->stream));
  uint64_t n = 0; double ms = 0, by = 0;
  if (strncmp(name, "host_", 5) == 0) {
    for (int i = 0; i < HT_COUNT; ++i)
      if (strcmp(name, kHostTimerName[i]) == 0) { n = c->host_n[i]; ms = c->host_ms[i]; }
    if (launches) *launches = n;
    if (total_ms) *total_ms = ms;
    if (bytes) *bytes = 0;
    return 0;
  }
  for (auto& t : c->launches) {
    if (t.name != name) continue;
    float x = 0;
    HIPCHK(hipEventElapsedTime(&x, t.a, t.b));
    ++n; ms += x; by += t.bytes;
  }
  if (launches) *launches = n;
  if (total_ms) *total_ms = ms;
  if (bytes) *bytes = by;
  return 0;
}

#if defined(PM_STEP_STAMPS) || defined(PM_MR_STAMPS) || defined(PM_ANSWER_STAMPS)
namespace pmh {
// Stamp builds: drain st, then append `hdr` and the first `count` words of
// `buf` to the file at `path`.
int dump_stamps(hipStream_t st, const char* path, const void* hdr, size_t hdr_bytes, const DevBuf& buf, uint64_t count) {
  HIPCHK(hipStreamSynchronize(st));
  std::vector<uint64_t> t(count);
  HIPCHK(hipMemcpy(t.data(), buf.p, count * 8, hipMemcpyDeviceToHost));
  static std::mutex mu;   // the teams' launching workers share the file
  std::lock_guard<std::mutex> lk(mu);
  if (FILE* f = fopen(path, "ab")) {
    fwrite(hdr, 1, hdr_bytes, f);
    fwrite(t.data(), 8, count, f);
    fclose(f);
  }
  return 0;
}
}  // namespace pmh
#endif

// ---------------------------------------------------------------------------
// leaf batches
// ---------------------------------------------------------------------------
extern "C" int pm_prf_batch(pm_ctx* c, const uint32_t rk[44], const uint64_t* tags, const uint64_t* xs,
                            uint64_t n, uint64_t* out) {
  if (n == 0) return 0;
  DevBuf drk, dt, dx, dout;
  CHK(drk.reserve(176)); CHK(dt.reserve(n * 8)); CHK(dx.reserve(n * 8)); CHK(dout.reserve(n * 8));
  hipStream_t st = c->stream;
  HIPCHK(hipMemcpyAsync(drk.p, rk, 176, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dt.p, tags, n * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dx.p, xs, n * 8, hipMemcpyHostToDevice, st));
  c->timed("prf", (double)n, [&] { pmk::prf_batch(st, drk.as<uint32_t>(), dt.as<uint64_t>(), dx.as<uint64_t>(), n, dout.as<uint64_t>()); });
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, dout.p, n * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
extern "C" int pm_l2_batch(pm_ctx* c, const float* q, const float* rows, uint64_t nrows, uint64_t dim,
                           float* out) {
  if (nrows == 0) return 0;
  if (dim == 0) return fail(PM_EINVAL, "dim must be > 0");
  DevBuf dq, dr, dout;
  CHK(dq.reserve(dim * 4)); CHK(dr.reserve(nrows * dim * 4)); CHK(dout.reserve(nrows * 4));
  hipStream_t st = c->stream;
  HIPCHK(hipMemcpyAsync(dq.p, q, dim * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dr.p, rows, nrows * dim * 4, hipMemcpyHostToDevice, st));
  c->timed("l2_rows", (double)nrows * dim * 4, [&] {
    pmk::l2_rows(st, dr.as<float>(), dim, nrows, nullptr, dq.as<float>(), (uint32_t)dim, dout.as<float>());
  });
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, dout.p, nrows * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
extern "C" int pm_ip_batch(pm_ctx* c, const uint32_t* q, const uint32_t* rows, uint64_t nrows, uint64_t dim,
                           uint32_t* per_row, uint32_t* sum) {
  if (dim == 0) return fail(PM_EINVAL, "dim must be > 0");
  DevBuf dq, dr, dpr, ds;
  CHK(dq.reserve(dim * 4)); CHK(dr.reserve(std::max<uint64_t>(1, nrows * dim * 4)));
  CHK(dpr.reserve(std::max<uint64_t>(4, nrows * 4))); CHK(ds.reserve(4));
  hipStream_t st = c->stream;
  HIPCHK(hipMemcpyAsync(dq.p, q, dim * 4, hipMemcpyHostToDevice, st));
  if (nrows) HIPCHK(hipMemcpyAsync(dr.p, rows, nrows * dim * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(ds.p, 0, 4, st));
  c->timed("ip_scan", (double)nrows * dim * 4, [&] {
    pmk::ip_rows(st, dr.as<uint32_t>(), nrows, dq.as<uint32_t>(), (uint32_t)dim, per_row ? dpr.as<uint32_t>() : nullptr,
                 ds.as<uint32_t>());
  });
  HIPCHK(hipGetLastError());
  if (per_row && nrows) HIPCHK(hipMemcpyAsync(per_row, dpr.p, nrows * 4, hipMemcpyDeviceToHost, st));
  uint32_t s = 0;
  HIPCHK(hipMemcpyAsync(&s, ds.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (sum) *sum = s;
  return 0;
}
extern "C" int pm_ip_bench(pm_ctx* c, uint64_t N, uint64_t D, uint32_t* sum, double* scan_ms) {
  return pm_ip_bench_shard(c, N, D, 0, N, sum, scan_ms);
}
extern "C" int pm_ip_bench_shard(pm_ctx* c, uint64_t Ntot, uint64_t D, uint64_t r0, uint64_t N, uint32_t* sum,
                                 double* scan_ms) {
  if (!c) return fail(PM_EINVAL, "NULL context");
  if (D == 0 || D % 4 || D > 4096) return fail(PM_EINVAL, "D must be a multiple of 4 and <= 4096");
  if (r0 > Ntot || N > Ntot - r0) return fail(PM_EINVAL, "shard rows past the fill's N");
  if (N == 0) {   // an empty shard adds nothing
    if (sum) *sum = 0;
    if (scan_ms) *scan_ms = 0.0;
    return 0;
  }
  DevBuf dv, dq, ds;
  CHK(dv.reserve(N * D * 4)); CHK(dq.reserve(D * 4)); CHK(ds.reserve(4));
  std::vector<uint32_t> q(D);
  for (uint64_t j = 0; j < D; ++j) q[j] = (uint32_t)j;
  hipStream_t st = c->stream;
  HIPCHK(hipMemcpyAsync(dq.p, q.data(), D * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(ds.p, 0, 4, st));
  pmk::ip_fill(st, dv.as<uint32_t>(), N, (uint32_t)D, r0);
  hipEvent_t a, b;
  HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
  HIPCHK(hipEventRecord(a, st));
  c->timed("ip_scan", (double)N * D * 4, [&] { pmk::ip_rows(st, dv.as<uint32_t>(), N, dq.as<uint32_t>(), (uint32_t)D, nullptr, ds.as<uint32_t>()); });
  HIPCHK(hipEventRecord(b, st));
  HIPCHK(hipGetLastError());
  uint32_t s = 0;
  HIPCHK(hipMemcpyAsync(&s, ds.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  if (sum) *sum = s;
  if (scan_ms) *scan_ms = ms;
  return 0;
}
