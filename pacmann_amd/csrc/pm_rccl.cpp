// pm_rccl.cpp — the library-native combine of the sharded loop: RCCL, resolved
// at run time (pm_rccl_*).
#include "pm_host.h"

// ---- the library-native combine: RCCL over xGMI (no Python on the step path) ----
// RCCL is resolved with dlopen on first use, not linked: the library loads on
// CPU-only machines, and a process that already mapped RCCL (torch's ROCm
// wheel ships librccl.so.1 too) shares that one copy (RTLD_NOLOAD by SONAME).
struct RcclApi {
  void* h = nullptr;
  std::string err;
  decltype(&ncclGetUniqueId) get_unique_id = nullptr;
  decltype(&ncclCommInitRank) comm_init_rank = nullptr;
  decltype(&ncclAllReduce) all_reduce = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclGetErrorString) error_string = nullptr;
  // the nonblocking forms (optional: an RCCL without them gets a watched blocking init)
  decltype(&ncclCommInitRankConfig) comm_init_rank_config = nullptr;
  decltype(&ncclCommGetAsyncError) get_async_error = nullptr;
  decltype(&ncclCommAbort) comm_abort = nullptr;
  decltype(&ncclGroupStart) group_start = nullptr;
  decltype(&ncclGroupEnd) group_end = nullptr;
  bool nonblocking() const { return comm_init_rank_config && get_async_error && comm_abort && group_start && group_end; }
};
static const RcclApi& rccl_api() {
  static const RcclApi api = [] {
    RcclApi a;
    a.h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!a.h) a.h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!a.h) a.h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!a.h) { const char* e = dlerror(); a.err = e ? e : "dlopen(librccl.so.1) failed"; return a; }
    a.get_unique_id = (decltype(a.get_unique_id))dlsym(a.h, "ncclGetUniqueId");
    a.comm_init_rank = (decltype(a.comm_init_rank))dlsym(a.h, "ncclCommInitRank");
    a.all_reduce = (decltype(a.all_reduce))dlsym(a.h, "ncclAllReduce");
    a.comm_destroy = (decltype(a.comm_destroy))dlsym(a.h, "ncclCommDestroy");
    a.error_string = (decltype(a.error_string))dlsym(a.h, "ncclGetErrorString");
    a.comm_init_rank_config = (decltype(a.comm_init_rank_config))dlsym(a.h, "ncclCommInitRankConfig");
    a.get_async_error = (decltype(a.get_async_error))dlsym(a.h, "ncclCommGetAsyncError");
    a.comm_abort = (decltype(a.comm_abort))dlsym(a.h, "ncclCommAbort");
    a.group_start = (decltype(a.group_start))dlsym(a.h, "ncclGroupStart");
    a.group_end = (decltype(a.group_end))dlsym(a.h, "ncclGroupEnd");
    if (!a.get_unique_id || !a.comm_init_rank || !a.all_reduce || !a.comm_destroy || !a.error_string)
      a.err = "librccl.so.1 lacks an NCCL entry point";
    return a;
  }();
  return api;
}
#define RCCLCHK(call)                                                                              \
  do {                                                                                             \
    const ncclResult_t r_ = (call);                                                                \
    if (r_ != ncclSuccess) return fail(PM_EHIP, std::string(#call ": ") + rccl_api().error_string(r_)); \
  } while (0)

// (rccl_timeout_s: g_rccl_timeout_s, with pm_set_option)
static double rccl_timeout_s() {
  const int o = g_rccl_timeout_s.load();
  if (o > 0) return o;
  const char* e = getenv("PM_RCCL_TIMEOUT_S");
  return e && atof(e) > 0 ? atof(e) : 120.0;
}

struct pm_rccl {
  int device = 0, nranks = 1, rank = 0;
  bool nonblocking = false;        // communicators made with config.blocking = 0: calls may return ncclInProgress
  std::vector<ncclComm_t> comms;   // one per lock-step team: a team's collectives never wait for another's
  bool aborted = false;
  void abort_all() {
    for (ncclComm_t& c : comms)
      if (c) { (void)(rccl_api().comm_abort ? rccl_api().comm_abort(c) : rccl_api().comm_destroy(c)); c = nullptr; }
    aborted = true;
  }
  ~pm_rccl() {
    for (ncclComm_t c : comms)
      if (c) (void)rccl_api().comm_destroy(c);
  }
};
// A call on a nonblocking communicator: ncclInProgress means "issued, not yet
// complete" -- poll the communicator's state until it settles (or the bound).
static ncclResult_t rccl_settle(const pm_rccl* r, ncclComm_t c, ncclResult_t res, double limit_s) {
  if (res != ncclInProgress || !r->nonblocking) return res;
  const auto t0 = Clock::now();
  ncclResult_t st = ncclInProgress;
  for (uint64_t polls = 0;; ++polls) {
    if (rccl_api().get_async_error(c, &st) != ncclSuccess) return ncclInternalError;
    if (st != ncclInProgress) return st;
    if (std::chrono::duration<double>(Clock::now() - t0).count() > limit_s) return ncclInProgress;
    // yield: RCCL's own proxy / init threads share the host cores with this poll
    std::this_thread::sleep_for(std::chrono::microseconds(polls < 100 ? 10 : 200));
  }
}

extern "C" int pm_rccl_unique_id(uint8_t id[PM_RCCL_ID_BYTES]) {
  if (!id) return fail(PM_EINVAL, "NULL argument");
  const RcclApi& a = rccl_api();
  if (!a.err.empty()) return fail(PM_EHIP, "RCCL unavailable: " + a.err);
  static_assert(sizeof(ncclUniqueId) == PM_RCCL_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId u;
  RCCLCHK(a.get_unique_id(&u));
  memcpy(id, &u, sizeof u);
  return 0;
}

// The teams' communicators, created within rccl_timeout_s() by ONE path (round
// 6): nonblocking inits (ncclCommInitRankConfig, config.blocking = 0) issued
// as one ncclGroupStart / ncclGroupEnd group -- NCCL's rule for several
// communicators created by one thread; round 5's ungrouped nonblocking inits
// never settled on the GPU box -- then each communicator's state polled with a
// yield (ncclCommGetAsyncError, 10-200 us sleeps) until it settles or the bound
// expires.  On an error or the bound every communicator is aborted
// (ncclCommAbort: RCCL's own init work ends), so no thread of this library is
// ever left inside RCCL; a rank whose peer never joined gets PM_ETIMEDOUT.
// An RCCL without the nonblocking API is refused (PM_EHIP): callers fall back.
static bool rccl_debug() {
  static const bool on = [] { const char* e = getenv("PM_RCCL_DEBUG"); return e && e[0] == '1'; }();
  return on;
}
extern "C" int pm_rccl_create(int device, int nranks, int rank, const uint8_t* ids, uint32_t nteams, pm_rccl** out) {
  if (!ids || !out || nteams == 0 || nranks < 1 || rank < 0 || rank >= nranks) return fail(PM_EINVAL, "bad argument");
  *out = nullptr;
  const double limit = rccl_timeout_s();
  // fault seams (tests): this rank's create fails at once (it never joins), or
  // its init never settles (the bounded wait runs out: PM_ETIMEDOUT after limit)
  static const int fault = [] { const char* e = getenv("PM_FAULT_RCCL_CREATE"); return e ? atoi(e) : -1; }();
  static const int fault_block = [] { const char* e = getenv("PM_FAULT_RCCL_BLOCK"); return e ? atoi(e) : -1; }();
  if (fault == rank) return fail(PM_EHIP, "injected fault (PM_FAULT_RCCL_CREATE)");
  if (fault_block == rank) {
    const auto t0 = Clock::now();
    while (std::chrono::duration<double>(Clock::now() - t0).count() <= limit)
      std::this_thread::sleep_for(std::chrono::milliseconds(5));
    return fail(PM_ETIMEDOUT, "RCCL communicators not ready after " + std::to_string((int)limit) +
                                  " s (injected: PM_FAULT_RCCL_BLOCK)");
  }
  const RcclApi& a = rccl_api();
  if (!a.err.empty()) return fail(PM_EHIP, "RCCL unavailable: " + a.err);
  if (!a.nonblocking()) return fail(PM_EHIP, "RCCL lacks the nonblocking init (ncclCommInitRankConfig / ncclCommAbort)");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<pm_rccl> r(new pm_rccl());
  r->device = device; r->nranks = nranks; r->rank = rank;
  r->comms.assign(nteams, nullptr);
  r->nonblocking = true;
  if (rccl_debug()) fprintf(stderr, "[pm] rccl_create rank %d/%d teams %u (grouped nonblocking inits)\n", rank, nranks, nteams);
  // every rank issues the teams' inits in the same order, as one group
  ncclResult_t gres = a.group_start();
  for (uint32_t t = 0; t < nteams && (gres == ncclSuccess || gres == ncclInProgress); ++t) {
    ncclUniqueId u;
    memcpy(&u, ids + (size_t)t * PM_RCCL_ID_BYTES, sizeof u);
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.blocking = 0;
    gres = a.comm_init_rank_config(&r->comms[t], nranks, u, rank, &cfg);
  }
  const ncclResult_t eres = a.group_end();
  if (rccl_debug()) fprintf(stderr, "[pm] rccl_create: group end %d (%s)\n", (int)eres, a.error_string(eres));
  if ((gres != ncclSuccess && gres != ncclInProgress) || (eres != ncclSuccess && eres != ncclInProgress)) {
    r->abort_all();
    return fail(PM_EHIP, std::string("ncclCommInitRankConfig: ") +
                             a.error_string(gres != ncclSuccess && gres != ncclInProgress ? gres : eres));
  }
  const auto t0 = Clock::now();
  for (uint32_t t = 0; t < nteams; ++t) {
    const double left = limit - std::chrono::duration<double>(Clock::now() - t0).count();
    const ncclResult_t st = rccl_settle(r.get(), r->comms[t], ncclInProgress, std::max(0.0, left));
    if (st == ncclInProgress) {
      r->abort_all();
      return fail(PM_ETIMEDOUT, "RCCL communicator " + std::to_string(t) + " not ready after " +
                                    std::to_string((int)limit) + " s (a peer rank did not join)");
    }
    if (st != ncclSuccess) {
      r->abort_all();
      return fail(PM_EHIP, std::string("RCCL communicator init: ") + a.error_string(st));
    }
  }
  if (rccl_debug())
    fprintf(stderr, "[pm] rccl_create: %u communicators ready in %.3f s\n", nteams,
            std::chrono::duration<double>(Clock::now() - t0).count());
  *out = r.release();
  return 0;
}

extern "C" void pm_rccl_destroy(pm_rccl* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  delete r;
}

extern "C" int pm_rccl_combine(void* user, uint32_t team, uint64_t* dev_words, uint64_t nwords, void* stream) {
  pm_rccl* r = (pm_rccl*)user;
  if (!r || r->comms.empty() || !dev_words) return fail(PM_EINVAL, "bad argument");
  if (r->aborted) return fail(PM_EHIP, "RCCL communicators were aborted");
  // in place, on the team's stream: ordered after the records' pack and before their read-back
  ncclComm_t c = r->comms[team % r->comms.size()];
  const ncclResult_t res = rccl_settle(r, c, rccl_api().all_reduce(dev_words, dev_words, nwords, ncclUint64, ncclSum, c,
                                                                   (hipStream_t)stream), rccl_timeout_s());
  if (res == ncclInProgress) return fail(PM_ETIMEDOUT, "ncclAllReduce not issued within the RCCL timeout");
  if (res != ncclSuccess) return fail(PM_EHIP, std::string("ncclAllReduce: ") + rccl_api().error_string(res));
  return 0;
}

// One 1-word all-reduce per team over the fresh communicators, on a private
// stream, completed within rccl_timeout_s(): every rank must see the sum
// nranks.  On a timeout or a wrong sum the communicators are aborted (their
// kernels return) and the handle refuses further combines.  Callers agree on
// the outcome over another channel (a MIN of the ranks' flags) before use.
extern "C" int pm_rccl_probe(pm_rccl* r) {
  if (!r || r->comms.empty()) return fail(PM_EINVAL, "bad argument");
  if (r->aborted) return fail(PM_EHIP, "RCCL communicators were aborted");
  HIPCHK(hipSetDevice(r->device));
  const uint32_t nt = (uint32_t)r->comms.size();
  DevBuf buf;
  CHK(buf.reserve(nt * 8));
  std::vector<uint64_t> one(nt, 1), got(nt, 0);
  hipStream_t st = nullptr;
  HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  struct Stream { hipStream_t s; ~Stream() { (void)hipStreamDestroy(s); } } guard{st};
  HIPCHK(hipMemcpyAsync(buf.p, one.data(), nt * 8, hipMemcpyHostToDevice, st));
  const double limit = rccl_timeout_s();
  if (rccl_debug()) fprintf(stderr, "[pm] rccl_probe: %u teams\n", nt);
  for (uint32_t t = 0; t < nt; ++t) {
    const int rc = pm_rccl_combine(r, t, buf.as<uint64_t>() + t, 1, st);
    if (rc) { r->abort_all(); return rc; }
  }
  if (rccl_debug()) fprintf(stderr, "[pm] rccl_probe: all-reduces issued\n");
  const auto t0 = Clock::now();
  for (;;) {
    const hipError_t e = hipStreamQuery(st);
    if (e == hipSuccess) break;
    if (e != hipErrorNotReady) { r->abort_all(); return fail(PM_EHIP, std::string("RCCL probe: ") + hipGetErrorString(e)); }
    if (std::chrono::duration<double>(Clock::now() - t0).count() > limit) {
      r->abort_all();
      (void)hipStreamSynchronize(st);   // the aborted communicators' kernels return
      return fail(PM_ETIMEDOUT, "RCCL probe all-reduce not complete after " + std::to_string((int)limit) + " s");
    }
    std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
  HIPCHK(hipMemcpy(got.data(), buf.p, nt * 8, hipMemcpyDeviceToHost));
  for (uint32_t t = 0; t < nt; ++t)
    if (got[t] != (uint64_t)r->nranks) {
      r->abort_all();
      return fail(PM_EHIP, "RCCL probe: team " + std::to_string(t) + " summed " + std::to_string(got[t]) + ", want " +
                               std::to_string(r->nranks));
    }
  return 0;
}
