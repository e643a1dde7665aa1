#define PM_HOST_TU 1
// pm_host.h — what more than one host file of libpacmann.so needs: the error
// macros, the device / pinned buffers, the context with its timing, and the
// declarations (namespace pmh) of what one host file uses of another.
// Included first by each pm_*.cpp; the .hip files do not see it.
#pragma once
#include "pm_internal.h"
#include "pm_aes.h"
#include "../../include/pacmann.h"

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types only: the functions are resolved at run time (rccl_api)

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

using namespace pm;

struct DevBuf;

// ---------------------------------------------------------------------------
// Functions and state used across host files.  Each is defined once, in the
// file named above its group; what one file alone uses is static there and
// is not listed.
// ---------------------------------------------------------------------------
namespace pmh {
// pm_ctx.cpp
int fail(int code, const std::string& msg);   // sets the calling thread's pm_last_error
// the option words of pm_set_option
extern std::atomic<int> g_verify_records;
extern std::atomic<int> g_device_loop;
extern std::atomic<int> g_rccl_timeout_s;
extern std::atomic<int> g_fault_drl_query;
extern std::atomic<int> g_stream_upload_only;   // pm_stream.cpp
int dump_stamps(hipStream_t st, const char* path, const void* hdr, size_t hdr_bytes, const DevBuf& buf, uint64_t count);   // stamp builds
}  // namespace pmh
using namespace pmh;

#define HIPCHK(x)                                                                         \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess)                                                                 \
      return fail(PM_EHIP, std::string(#x) + ": " + hipGetErrorString(e_));               \
  } while (0)
#define CHK(x)            \
  do {                    \
    int r_ = (x);         \
    if (r_ != 0) return r_; \
  } while (0)

// ---------------------------------------------------------------------------
// context, device buffers, timing
// ---------------------------------------------------------------------------
struct DevBuf {
  void* p = nullptr;
  size_t n = 0;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int reserve(size_t bytes) {
    if (bytes <= n) return 0;
    if (p) { (void)hipFree(p); p = nullptr; n = 0; }
    if (bytes == 0) return 0;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return fail(PM_ENOMEM, "hipMalloc(" + std::to_string(bytes) + "): " + hipGetErrorString(e));
    n = bytes;
    return 0;
  }
  template <class T> T* as() const { return (T*)p; }
};
// Pinned host memory the GPU reads (step descriptor) and writes (results)
// zero-copy.  It must be fine-grained (coherent): with the default
// coarse-grained allocation the GPU may serve the descriptor from a stale L2
// line and the host may read result rows before the device writes land.
struct HostBuf {
  void* p = nullptr;
  size_t n = 0;
  ~HostBuf() { if (p) (void)hipHostFree(p); }
  int reserve(size_t bytes) {
    if (bytes <= n) return 0;
    if (p) { (void)hipHostFree(p); p = nullptr; n = 0; }
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocCoherent | hipHostMallocMapped);
    if (e != hipSuccess) return fail(PM_ENOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    memset(p, 0, bytes);   // no stale step token (PmOutHdr::token is never 0)
    n = bytes;
    return 0;
  }
  template <class T> T* as() const { return (T*)p; }
};

// Host wall-clock accumulators, read back as "host_*" through pm_timing_get.
// The "host_path_match*" entries count the hint-search kernel each step launched
// (k_match / k_match_part / k_match_part8; total_ms 0); the other "host_path_*"
// the step's remaining kernels by the form the step's plan launched (pmk::step_plan, pmk::FORM_*;
// total_ms 0 unless noted): "step" the fused k_step<W>, total_ms = the sum of
// its gather helpers per sub-query (nhelp; a count, not a time); "resolve_lds"
// / "resolve_g" k_resolve<true> / <false>; "mr_s2" / "mr_s4" / "mr_general"
// k_match_resolve_s<2,256> / <4,256> / k_match_resolve; "gather" k_gather<W>;
// "answer_p5" / "answer_p" / "answer_s" / "answer_g" k_answer_p5 / k_answer_p /
// k_answer_s<W,NT> / k_answer<W>.  "host_answer_packed" counts, beside
// "answer_p5" / "answer_p", those of their launches that gathered the server's
// packed row image (k_answer_p5k / k_answer_pk).  "host_prep_sets" counts the
// re-preprocessing launch sets of the serving loops, with total_ms = the number
// of clients they folded (a count, not a time).
// The "host_records_*" entries count the sharded loop's record checks
// (pm_set_option "verify_records"): answered records equal to the graph's row
// and the reference-order L2 (verified) or not (bad); unanswered ids explained
// by the batch layer's overflow drop (dropped), by a failed sub-query of this
// rank (failed), by another rank's sub-query (peer), or not at all (unexplained).
// "host_fold_*" count the maintenance fold launches by form (pmk::fold_form):
// "rot512" / "rot1024" k_prep_fold_rot at CS 512 / 1,024, "rot512p" the same
// kernel at CS 512 over a packed image (FOLD_ROT512P), "rot512q" over a
// bit-packed one (FOLD_ROT512Q; its total_ms adds up the slices each launch
// folded, a count: 9 for SIFT1M's rows, 11 with 12-bit coordinates or 20-bit
// ids alone); "other" every launch
// that is not a rotated one, which "pipe" (k_prep_fold_pipe), "blk"
// (k_prep_fold_blk, one count for its full-width and remainder launches) and
// "gather" (the unblocked k_prep_fold<W>, E < 4 included) split by kernel
// family: other == pipe + blk + gather.  "host_dev_steps" / "host_dev_queries"
// the shared steps and session queries the device loop served (pm_drl.hip).
// "host_knn_batch_fallback": the host remainder of pm_search_knn_batch's device
// path, one entry per call that re-ran queries whose search drew from the id stream.
// "host_gvi_group": the wall time of pm_graph_group_get_vertex_info, one entry per
// call; "host_gvi_group_steps": the shared steps those calls launched (a count),
// both on the context of the group's first session.
// "host_server_answer_packed": the k_server_answer_parts launches of
// pm_batchpir_server_answer that gathered the packed row image (a count).
// "host_client_begin" / "host_client_finish": the wall time of pm_batchpir_client_begin /
// _finish, one entry per call that ran (a refused call counts nothing).
// "host_prep_stream": the wall time of a streamed preprocessing from pm_batchpir_prep_stream_begin to _end, one
// entry per completed stream; "host_prep_stream_windows": the sub-windows its rows went up in (a count).
enum HostTimer : int { HT_STEP_LAUNCH, HT_STEP_WAIT, HT_STEP_POST, HT_BATCH_QUERY, HT_GVI_PARSE, HT_SEARCH_KNN, HT_KNN_INIT, HT_KNN_BATCH, HT_KNN_UPDATE, HT_KNN_FINAL, HT_WAIT_FIRST, HT_WAIT_ALL, HT_ROWS_SEEN, HT_ROWS_TORN, HT_WAIT_DONE, HT_COMBINE, HT_COMBINE_TURN, HT_PATH_MATCH, HT_PATH_MATCH_PART, HT_PATH_MATCH_PART8, HT_PREP_SETS, HT_REC_VERIFIED, HT_REC_BAD, HT_REC_DROPPED, HT_REC_FAILED, HT_REC_PEER, HT_REC_UNEXPLAINED, HT_FOLD_ROT512, HT_FOLD_ROT1024, HT_FOLD_OTHER, HT_FOLD_PIPE, HT_FOLD_BLK, HT_FOLD_GATHER, HT_FOLD_ROT512P, HT_FOLD_ROT512Q, HT_DEV_STEPS, HT_DEV_QUERIES, HT_KNN_BATCH_FALLBACK, HT_PATH_STEP, HT_PATH_RESOLVE_LDS, HT_PATH_RESOLVE_G, HT_PATH_MR_S2, HT_PATH_MR_S4, HT_PATH_MR_GENERAL, HT_PATH_GATHER, HT_PATH_ANSWER_P5, HT_PATH_ANSWER_P, HT_PATH_ANSWER_S, HT_PATH_ANSWER_G, HT_ANSWER_PACKED, HT_GVI_GROUP, HT_GVI_GROUP_STEPS, HT_SERVER_ANSWER_PACKED, HT_CLIENT_BEGIN, HT_CLIENT_FINISH, HT_PREP_STREAM, HT_PREP_STREAM_WINDOWS, HT_COUNT };
static const char* const kHostTimerName[HT_COUNT] = {"host_step_launch", "host_step_wait", "host_step_post", "host_batch_query", "host_gvi_parse", "host_search_knn", "host_knn_init", "host_knn_batch", "host_knn_update", "host_knn_final", "host_wait_first_token", "host_wait_all_tokens", "host_rows_seen", "host_rows_torn", "host_wait_done", "host_combine", "host_combine_turn", "host_path_match", "host_path_match_part", "host_path_match_part8", "host_prep_sets", "host_records_verified", "host_records_bad", "host_records_dropped", "host_records_failed", "host_records_peer", "host_records_unexplained", "host_fold_rot512", "host_fold_rot1024", "host_fold_other", "host_fold_pipe", "host_fold_blk", "host_fold_gather", "host_fold_rot512p", "host_fold_rot512q", "host_dev_steps", "host_dev_queries", "host_knn_batch_fallback", "host_path_step", "host_path_resolve_lds", "host_path_resolve_g", "host_path_mr_s2", "host_path_mr_s4", "host_path_mr_general", "host_path_gather", "host_path_answer_p5", "host_path_answer_p", "host_path_answer_s", "host_path_answer_g", "host_answer_packed", "host_gvi_group", "host_gvi_group_steps", "host_server_answer_packed", "host_client_begin", "host_client_finish", "host_prep_stream", "host_prep_stream_windows"};
static_assert(HT_PATH_ANSWER_G - HT_PATH_STEP + 1 == pmk::FORM_COUNT, "one counter per step form, in the order of pmk::FORM_*");

struct TimedLaunch { std::string name; hipEvent_t a, b; double bytes; };

struct pm_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int timing = 0;   // 0 off, 1 preprocessing / leaf kernels, 2 also the per-step kernels,
                    // 3 as 2 with the shared steps' kernels timed on every kSampleSteps-th step
  // timing 3: whether the current shared step's kernels carry events (group_step)
  bool sample_now = true;
  uint64_t sample_ctr = 0;
  bool no_fuse = false;      // PM_NO_FUSE=1: the three step kernels even when k_step fits
  bool no_split = false;     // PM_NO_SPLIT=1: k_answer gathers wide sets itself (no k_gather)
  bool no_guess = false;     // PM_NO_GUESS=1: k_step answers do not start before their resolution
  bool step_spec = false;    // PM_STEP_SPEC=1: k_step keeps its speculation record (pm_batchpir_step_spec)
  bool verify_rows = false;  // PM_VERIFY_ROWS=1: re-read each step's results after the stream drains
  bool debug_cache = false;  // PM_DEBUG_CACHE=1: check cached answers against the slot's first answer
  bool log_steps = false;    // PM_LOG_STEPS=1: one stderr line per sub-query per step
  bool debug_sync = false;   // PM_DEBUG_SYNC=1: synchronise after every launch (fault triage)
  // Maintenance: the replacement rows (HBM copies, independent of the PRF
  // tables and the fold) run on a side stream beside k_prep_offsets
  // (PM_REPL_SIDE=0: after the fold on the one stream; timed runs keep that
  // order so every launch carries its own events)
  bool repl_side = true;
  hipStream_t side = nullptr;
  hipEvent_t side_ev[2] = {};
  std::mutex side_mu;
  // Result rows vs their header checksum when the token is first seen
  // (PmOutHdr::csum): 0 = no check, 1 = count a mismatch ("host_rows_torn")
  // and fail the step, 2 = count it and wait for the row to match (PM_ROWS_CHECK)
  int rows_check = 2;
  std::vector<uint64_t> hash_mult;   // row_hash_mult(w) for every word a row can have
  // Step completion (result publication): an event recorded
  // after the step's last kernel, with a system-scope release, so that once
  // hipEventQuery reports it, every result byte the step wrote into pinned
  // memory is visible to the host (HIP event semantics; the header tokens
  // alone give no such order).  One worker queries the runtime, the others read
  // an atomic.
  // Steps of several engines (or a session's own steps beside its group's)
  // can share one context, so completions are counted per context: record_done
  // returns the step's sequence number (counted after the record), done_seen
  // is the highest one known complete.  A later record of the event covers
  // the earlier steps of the stream.
  // PM_PUBLISH_WAIT=0: the token + row-hash acceptance alone (diagnostics).
  // Each step's completion has an event of its own in a ring (step seq uses
  // done_ring[seq % kDoneRing]): a waiter for step seq queries that step's
  // event, not the newest one, so it never waits for steps recorded after its
  // own (a slot re-recorded 64 steps later still completes after it: one stream).
  bool publish_wait = true;
  static constexpr uint32_t kDoneRing = 64;
  hipEvent_t done_ev = nullptr;   // done_ring[0] (creation check)
  hipEvent_t done_ring[kDoneRing] = {};
  std::atomic<uint64_t> done_rec{0}, done_seen{0};
  std::mutex done_mu, rec_mu;
  uint64_t record_done(hipStream_t st) {
    if (!publish_wait) return 0;
    std::lock_guard<std::mutex> lk(rec_mu);
    const uint64_t seq = done_rec.load(std::memory_order_relaxed) + 1;
    (void)hipEventRecord(done_ring[seq % kDoneRing], st);
    done_rec.store(seq, std::memory_order_release);
    return seq;
  }
  std::string last_kernel;
  // host-side wall-clock accumulators ("host_*" names in pm_timing_get)
  uint64_t host_n[HT_COUNT] = {};
  double host_ms[HT_COUNT] = {};
  void host_add(HostTimer t, double ms) { host_n[t]++; host_ms[t] += ms; }
  // the counter of a step launch: the plan's form at `stage` (pmk::MATCH_* at STAGE_MATCH, else pmk::FORM_*)
  static HostTimer step_counter(int stage, int form) {
    if (stage != pmk::STAGE_MATCH) return (HostTimer)(HT_PATH_STEP + form);
    return form == pmk::MATCH_PART8 ? HT_PATH_MATCH_PART8 : form == pmk::MATCH_PART ? HT_PATH_MATCH_PART : HT_PATH_MATCH;
  }
  std::vector<TimedLaunch> launches;
  std::vector<hipEvent_t> pool;
  hipEvent_t ev() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
  }
  // Bracket a launch with events on the stream it runs on (when enabled).
  template <class F> void timed(const char* name, double bytes, F&& f, int level = 1) {
    last_kernel = name;
    if (debug_sync) {
      f();
      hipError_t e = hipStreamSynchronize(stream);
      if (e != hipSuccess) fprintf(stderr, "[pm] kernel %s failed: %s\n", name, hipGetErrorString(e));
      return;
    }
    if (timing < level) { f(); return; }
    TimedLaunch t{name, ev(), ev(), bytes};
    (void)hipEventRecord(t.a, stream);
    f();
    (void)hipEventRecord(t.b, stream);
    launches.push_back(t);
  }
  // The same for launchers that attach the events to the kernel's own dispatch
  // packet (hipExtLaunchKernelGGL): no marker latency around short kernels.
  template <class F> void timed_ext(const char* name, double bytes, F&& f, int level) {
    last_kernel = name;
    if (debug_sync) { timed(name, bytes, [&] { f(pmk::PmEvents{}); }, level); return; }
    if (timing < level || (timing == 3 && level == 2 && !sample_now)) { f(pmk::PmEvents{}); return; }
    TimedLaunch t{name, ev(), ev(), bytes};
    f(pmk::PmEvents{t.a, t.b});
    launches.push_back(t);
  }
  ~pm_ctx() {
    for (auto& t : launches) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
    for (auto e : pool) (void)hipEventDestroy(e);
    for (auto e : done_ring) if (e) (void)hipEventDestroy(e);
    for (auto e : side_ev) if (e) (void)hipEventDestroy(e);
    if (side) (void)hipStreamDestroy(side);
    if (stream) (void)hipStreamDestroy(stream);
  }
};
// ---------------------------------------------------------------------------
// pm_build.cpp: the exact kNN device path, shared with pm_cluster.cpp
// (pm_kmeans' assignment and pm_cluster_search's probe are kNN calls with the
// centroids as base).
// ---------------------------------------------------------------------------
struct KnnDev {   // device copies for the prefilter + re-rank
  DevBuf x, xb, xl, xn, mx;   // f32 rows, bf16 rows (exact: hi), exact: lo, norms, exact: the largest norm's bits
  uint32_t dp = 0;
};
struct KnnOut {   // knn_device's buffers (see there)
  DevBuf cand, out, dist, len, tau, list, nlist, pref, eps;
  bool stages = false;
  uint64_t nl = 0;
};
extern const char* const kWideDimText;   // "dim must be in [1, 1024]"
bool wide_dim_ok(uint64_t dim);
int knn_upload(pm_ctx* c, const float* v, uint64_t n, uint32_t dim, KnnDev& d, bool exact, bool wide = false,
               hipMemcpyKind kind = hipMemcpyHostToDevice);
int knn_device(pm_ctx* c, const KnnDev& B, uint64_t n, const KnnDev& Q, uint64_t nq, uint32_t dim, uint32_t K,
               bool self_base, bool want_dist, bool exact, KnnOut& o, uint64_t* fallback,
               uint32_t top = pmk::knn_top());

using Clock = std::chrono::steady_clock;
static inline double ms_since(Clock::time_point t) {
  return std::chrono::duration<double, std::milli>(Clock::now() - t).count();
}
