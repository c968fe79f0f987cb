// ssim_comm.cpp -- the RCCL all-reduce of the C ABI (rmgr_ssim_hip_comm_*): one process per GPU, per-image sums combined across ranks.
#include "ssim_context.h"
#include <dlfcn.h>

#include <atomic>
#include <condition_variable>
#include <string>
#include <thread>

// ---- RCCL, loaded lazily so that single-GPU users carry no dependency on it ----
//
// Every step that can wait for something outside this process has a DEADLINE ($RMGR_SSIM_HIP_COMM_TIMEOUT_S, default
// 30 s): loading the library, the bootstrap behind ncclGetUniqueId, the rendezvous of ncclCommInitRank, the enqueue of the
// all-reduce, the teardown.  The reference turns a failed worker into a bounded ECHILD return (src/ssim.cpp:1094-1097);
// the GPU-era counterpart of "a worker failed" is "a rank never arrived", and that must come back as an errno
// (ETIMEDOUT) too, not as a hang.  Mechanics: library load, ncclGetUniqueId and the communicator's creation run on a helper
// thread the caller waits for with a timeout; the communicator is requested NON-BLOCKING (ncclCommInitRankConfig, blocking
// = 0), its state polled with ncclCommGetAsyncError and, past the deadline, torn down with ncclCommAbort by the helper.  The
// RCCL builds of this image (2.26.6, 2.27.7) run the rendezvous inside ncclCommInitRankConfig all the same (the helper's log
// shows the call returning only when the communicator is ready), so there the helper's timeout is the bound that acts: a
// helper that never returns is abandoned -- the process keeps one parked thread; nothing it owns lives on the caller's stack.
namespace ssim_host {
namespace {

struct Rccl {
    void* handle;
    char  path[256];          // what dlopen() resolved (diagnostics: rmgr_ssim_hip_comm_describe)
    int   version;
    ncclResult_t (*GetVersion)(int*);
    ncclResult_t (*GetUniqueId)(ncclUniqueId*);
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int);
    ncclResult_t (*CommInitRankConfig)(ncclComm_t*, int, ncclUniqueId, int, ncclConfig_t*);     // optional
    ncclResult_t (*CommGetAsyncError)(ncclComm_t, ncclResult_t*);                               // optional
    ncclResult_t (*CommAbort)(ncclComm_t);                                                      // optional
    ncclResult_t (*CommFinalize)(ncclComm_t);                                                   // optional
    ncclResult_t (*CommCount)(const ncclComm_t, int*);
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
    ncclResult_t (*CommDestroy)(ncclComm_t);
};

template <typename F> void sym(void* h, const char* name, F& f) { f = reinterpret_cast<F>(dlsym(h, name)); }

// Which librccl: $RMGR_SSIM_HIP_RCCL_LIB if set; else the SONAME first -- a process that already carries an RCCL (a host
// framework that bundles its own copy next to its own HIP runtime, e.g. a PyTorch wheel) must get THAT copy back, not a
// second RCCL bound to a second HIP runtime -- then the development name and ROCm's default location.
// NEVER waits: the first caller loads (dlopen + dlsym, on whichever thread that is -- normally a communicator helper); while that
// is in progress every other caller gets NULL (-> ENOSYS / "not loadable yet") instead of queueing behind a load that an
// abandoned helper might be stuck in (std::call_once made every later caller wait without a bound).
// path_override: $RMGR_SSIM_HIP_RCCL_LIB as the CALLER's thread read it (helpers do not call getenv: the host process -- Python --
// may be changing its environment concurrently).
enum { RCCL_UNLOADED = 0, RCCL_LOADING = 1, RCCL_READY = 2, RCCL_ABSENT = 3 };
Rccl             g_rccl_api;
std::atomic<int> g_rccl_state(RCCL_UNLOADED);

// wait_for_load (communicator helpers only -- their caller bounds THEM): sleep through another thread's load instead of reporting NULL.
Rccl* rccl(const char* path_override = NULL, bool use_env = true, bool wait_for_load = false)
{
    for (;;) {
        const int st = g_rccl_state.load(std::memory_order_acquire);
        if (st == RCCL_READY) return &g_rccl_api;
        if (st == RCCL_ABSENT) return NULL;
        if (st == RCCL_LOADING) {
            if (!wait_for_load) return NULL;
            std::this_thread::sleep_for(std::chrono::milliseconds(1));
            continue;
        }
        int expected = RCCL_UNLOADED;
        if (g_rccl_state.compare_exchange_strong(expected, RCCL_LOADING)) break;
    }
    Rccl& api = g_rccl_api;
    memset(&api, 0, sizeof(api));
    const char* names[] = {path_override ? path_override : (use_env ? getenv("RMGR_SSIM_HIP_RCCL_LIB") : NULL), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (size_t i = 0; i < sizeof(names) / sizeof(names[0]) && !api.handle; ++i)
        if (names[i] && names[i][0]) api.handle = dlopen(names[i], RTLD_NOW | RTLD_LOCAL);
    if (api.handle) {
        sym(api.handle, "ncclGetVersion", api.GetVersion);
        sym(api.handle, "ncclGetUniqueId", api.GetUniqueId);
        sym(api.handle, "ncclCommInitRank", api.CommInitRank);
        sym(api.handle, "ncclCommInitRankConfig", api.CommInitRankConfig);
        sym(api.handle, "ncclCommGetAsyncError", api.CommGetAsyncError);
        sym(api.handle, "ncclCommAbort", api.CommAbort);
        sym(api.handle, "ncclCommFinalize", api.CommFinalize);
        sym(api.handle, "ncclCommCount", api.CommCount);
        sym(api.handle, "ncclAllReduce", api.AllReduce);
        sym(api.handle, "ncclCommDestroy", api.CommDestroy);
        if (!api.GetUniqueId || !api.CommInitRank || !api.AllReduce || !api.CommDestroy || !api.CommCount) { dlclose(api.handle); api.handle = NULL; }
    }
    if (api.handle) {
        if (api.GetVersion) (void)api.GetVersion(&api.version);
        Dl_info info;
        if (dladdr(reinterpret_cast<void*>(api.AllReduce), &info) && info.dli_fname) snprintf(api.path, sizeof(api.path), "%s", info.dli_fname);
    }
    g_rccl_state.store(api.handle ? RCCL_READY : RCCL_ABSENT, std::memory_order_release);
    return api.handle ? &api : NULL;
}

int map_nccl(ncclResult_t r)
{
    switch (r) {
    case ncclSuccess:          return 0;
    case ncclInvalidArgument:
    case ncclInvalidUsage:     return EINVAL;
    case ncclInProgress:       return ETIMEDOUT;     // only ever surfaces once a deadline has passed
    case ncclSystemError:
    case ncclUnhandledCudaError:
    case ncclInternalError:
    default:                   return ECHILD;
    }
}

typedef std::chrono::steady_clock Clock;

double comm_timeout_s()
{
    if (const char* e = getenv("RMGR_SSIM_HIP_COMM_TIMEOUT_S")) {
        const double v = atof(e);
        if (v > 0.0) return v;
    }
    return 30.0;
}

Clock::time_point deadline_from_now(double seconds)
{
    return Clock::now() + std::chrono::duration_cast<Clock::duration>(std::chrono::duration<double>(seconds));
}

// $RMGR_SSIM_HIP_COMM_DEBUG=1: the helper thread reports its steps on stderr (where a stalled bootstrap stalled).  The variable
// is read on the CALLER's thread (comm_debug_wanted) and travels in the job: helpers never call getenv.
bool comm_debug_wanted()
{
    const char* e = getenv("RMGR_SSIM_HIP_COMM_DEBUG");
    return e && atoi(e) != 0;
}

void comm_debug(bool on, const char* what, double seconds = -1.0)
{
    if (!on) return;
    if (seconds >= 0.0) fprintf(stderr, "[rmgr-ssim comm] %s (%.3f s)\n", what, seconds);
    else                fprintf(stderr, "[rmgr-ssim comm] %s\n", what);
    fflush(stderr);
}

double seconds_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// A job for the helper thread.  Everything the helper touches lives in this heap block (shared with the caller through a
// shared_ptr), so a helper that outlives its caller's patience has nothing dangling to write to.
struct CommJob {
    std::mutex m;
    std::condition_variable cv;
    bool done;                     // the helper has finished (under m)
    bool abandoned;                // the caller has given up waiting (under m): whatever the helper still produces is the helper's to clean up
    std::atomic<bool> cancel;      // the polling loop's view of `abandoned`
    int rc;
    // inputs
    int device, rank_count, rank;
    bool want_id, nonblocking_ok;
    bool debug;                    // $RMGR_SSIM_HIP_COMM_DEBUG, read by the caller
    std::string rccl_path;         // $RMGR_SSIM_HIP_RCCL_LIB, read by the caller ("" = unset)
    ncclUniqueId id;
    // outputs
    ncclComm_t comm;
    bool nonblocking;
    CommJob() : done(false), abandoned(false), cancel(false), rc(0), device(0), rank_count(0), rank(0), want_id(false), nonblocking_ok(true), debug(false), comm(NULL), nonblocking(false) { memset(&id, 0, sizeof(id)); }
};

void comm_job_body(const std::shared_ptr<CommJob>& j)
{
    const Clock::time_point t0 = Clock::now();
    int rc = 0;
    comm_debug(j->debug, "helper: loading librccl");
    Rccl* r = rccl(j->rccl_path.empty() ? NULL : j->rccl_path.c_str(), false, true);      // may load (and page in) half a gigabyte of library; no getenv here
    comm_debug(j->debug, r ? r->path : "helper: no usable librccl", seconds_since(t0));
    if (!r) rc = ENOSYS;
    else if (j->want_id) { rc = map_nccl(r->GetUniqueId(&j->id)); comm_debug(j->debug, "helper: ncclGetUniqueId returned", seconds_since(t0)); }
    else if (hipSetDevice(j->device) != hipSuccess) { (void)hipGetLastError(); rc = ENODEV; }
    else {
        ncclResult_t res;
        if (j->nonblocking_ok && r->CommInitRankConfig && r->CommGetAsyncError && r->CommAbort) {
            ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
            cfg.blocking = 0;
            res = r->CommInitRankConfig(&j->comm, j->rank_count, j->id, j->rank, &cfg);
            char msg[96];
            snprintf(msg, sizeof(msg), "helper: ncclCommInitRankConfig(blocking = 0) returned %d", (int)res);
            comm_debug(j->debug, msg, seconds_since(t0));
            // An error here is final (no second attempt with the plain call: the id's rendezvous has been used).
            if (res == ncclSuccess || res == ncclInProgress) {
                j->nonblocking = true;
                for (;;) {                                   // the rendezvous proceeds on RCCL's own thread
                    ncclResult_t state = ncclSuccess;
                    const ncclResult_t g = r->CommGetAsyncError(j->comm, &state);
                    if (g != ncclSuccess) { res = g; break; }
                    if (state != ncclInProgress) { res = state; break; }
                    if (j->cancel.load()) { res = ncclInProgress; break; }      // the caller's deadline passed
                    std::this_thread::sleep_for(std::chrono::microseconds(200));
                }
                comm_debug(j->debug, res == ncclSuccess ? "helper: communicator ready" : res == ncclInProgress ? "helper: deadline passed, aborting the communicator" : "helper: init failed, aborting the communicator", seconds_since(t0));
                if (res != ncclSuccess && j->comm) { (void)r->CommAbort(j->comm); j->comm = NULL; comm_debug(j->debug, "helper: ncclCommAbort returned", seconds_since(t0)); }
            }
        } else {
            res = r->CommInitRank(&j->comm, j->rank_count, j->id, j->rank);
            comm_debug(j->debug, "helper: ncclCommInitRank returned", seconds_since(t0));
        }
        if (res != ncclSuccess) j->comm = NULL;
        rc = map_nccl(res);
    }
    std::unique_lock<std::mutex> lk(j->m);
    j->rc = rc;
    j->done = true;
    const bool orphan = j->abandoned && j->comm != NULL;     // finished after the caller left: nobody will ever own this communicator
    lk.unlock();
    j->cv.notify_all();
    if (orphan) {
        if (r && r->CommAbort) (void)r->CommAbort(j->comm);
        j->comm = NULL;
        comm_debug(j->debug, "helper: late communicator aborted", seconds_since(t0));
    }
}

// Runs the job on a helper thread and waits for it until the deadline.  Past it the caller returns ETIMEDOUT AT ONCE: the
// helper is told to give up -- its polling loop aborts the half-built communicator, which can itself take seconds while
// RCCL's bootstrap thread winds down -- and is left to finish that on its own (detached; it owns everything it touches).
int run_comm_job(const std::shared_ptr<CommJob>& j, double timeout_s)
{
    j->debug = comm_debug_wanted();                           // the environment is read HERE, on the caller's thread
    if (const char* e = getenv("RMGR_SSIM_HIP_RCCL_LIB")) { try { j->rccl_path = e; } catch (...) { return ENOMEM; } }
    std::thread t;
    try { t = std::thread(comm_job_body, j); } catch (...) { return EAGAIN; }
    std::unique_lock<std::mutex> lk(j->m);
    if (j->cv.wait_until(lk, deadline_from_now(timeout_s), [&] { return j->done; })) { lk.unlock(); t.join(); return j->rc; }
    j->abandoned = true;
    j->cancel.store(true);
    lk.unlock();
    t.detach();
    return ETIMEDOUT;
}

// Waits for a non-blocking communicator's last call to leave the "in progress" state.
int comm_wait_ready(Rccl* r, rmgr_ssim_hip_Context* c, ncclResult_t first)
{
    if (first != ncclInProgress) return map_nccl(first);
    if (!c->comm_nonblocking || !r->CommGetAsyncError) return map_nccl(first);
    const Clock::time_point deadline = deadline_from_now(comm_timeout_s());
    for (;;) {
        ncclResult_t state = ncclSuccess;
        const ncclResult_t g = r->CommGetAsyncError(c->comm, &state);
        if (g != ncclSuccess) return map_nccl(g);
        if (state != ncclInProgress) return map_nccl(state);
        if (Clock::now() > deadline) return ETIMEDOUT;
        std::this_thread::yield();
    }
}

} // namespace

static void comm_abort(Rccl* r, rmgr_ssim_hip_Context* c)
{
    if (!c->comm) return;
    if (r && r->CommAbort) (void)r->CommAbort(c->comm);
    c->comm = NULL;               // without ncclCommAbort the handle is leaked rather than destroyed: ncclCommDestroy would wait for the peers
    c->comm_nonblocking = false;
    c->comm_ranks = 0;
}

// rmgr_ssim_hip_synchronize() / _destroy() of a context that owns a communicator: the stream may hold an all-reduce whose peers never
// launch theirs, and hipStreamSynchronize() would then wait forever.  So the wait POLLS, and it bounds the collectives only: each
// queued all-reduce sits between two events (comm_allreduce_sums); while the oldest outstanding one has not had its turn (its
// `begin` event is not complete) ordinary work is running and no clock ticks; from the moment `begin` completes that collective
// has $RMGR_SSIM_HIP_COMM_TIMEOUT_S to finish; past that the communicator is aborted (ncclCommAbort releases the kernel that spins
// on the missing peers), the wait for that kernel to leave is itself bounded by another such interval, and the caller gets
// ETIMEDOUT.  Without ncclCommAbort nothing can release the kernel: ETIMEDOUT is returned with the stream left as it is.  The
// poll sleeps (50 us, doubling up to 1 ms) instead of spinning.
static hipEvent_t comm_take_event(rmgr_ssim_hip_Context* c)
{
    hipEvent_t e = NULL;
    if (!c->spare_events.empty()) { e = c->spare_events.back(); c->spare_events.pop_back(); return e; }
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return NULL; }
    return e;
}

void comm_forget_collectives(rmgr_ssim_hip_Context* c)
{
    while (!c->collectives.empty()) {
        c->spare_events.push_back(c->collectives.front().begin);
        c->spare_events.push_back(c->collectives.front().end);
        c->collectives.pop_front();
    }
}

int comm_bounded_sync(rmgr_ssim_hip_Context* c)
{
    const double limit = comm_timeout_s();
    std::chrono::microseconds nap(50);
    for (;;) {
        while (!c->collectives.empty()) {                        // retire what has completed
            const hipError_t e = hipEventQuery(c->collectives.front().end);
            if (e == hipErrorNotReady) break;
            if (e != hipSuccess) { (void)hipGetLastError(); return map_hip_error(e); }
            c->spare_events.push_back(c->collectives.front().begin);
            c->spare_events.push_back(c->collectives.front().end);
            c->collectives.pop_front();
        }
        if (c->collectives.empty()) {                            // nothing left on the stream can wait for a peer
            HIP_TRY(hipStreamSynchronize(c->stream));
            return 0;
        }
        rmgr_ssim_hip_Context_::Collective& k = c->collectives.front();
        if (!k.started) {
            const hipError_t e = hipEventQuery(k.begin);
            if (e == hipSuccess) { k.started = true; k.since = Clock::now(); }
            else if (e != hipErrorNotReady) { (void)hipGetLastError(); return map_hip_error(e); }
        } else if (std::chrono::duration<double>(Clock::now() - k.since).count() > limit) {
            Rccl* r = rccl();
            const bool can_abort = r && r->CommAbort;
            const hipEvent_t stuck = k.end;
            comm_abort(r, c);
            if (can_abort) {                                    // the aborted collective's kernel exits: wait for it, bounded
                const Clock::time_point until = deadline_from_now(limit);
                while (hipEventQuery(stuck) == hipErrorNotReady && Clock::now() < until) std::this_thread::sleep_for(std::chrono::microseconds(200));
            }
            (void)hipGetLastError();
            comm_forget_collectives(c);
            return ETIMEDOUT;
        }
        std::this_thread::sleep_for(nap);
        if (nap < std::chrono::microseconds(1000)) nap *= 2;
    }
}

} // namespace ssim_host

using namespace ssim_host;

extern "C" rmgr_int32_t rmgr_ssim_hip_comm_get_unique_id(unsigned char id[RMGR_SSIM_HIP_COMM_ID_BYTES]) RMGR_NOEXCEPT
{
    static_assert(sizeof(ncclUniqueId) == RMGR_SSIM_HIP_COMM_ID_BYTES, "ncclUniqueId size");
    if (!id) return EINVAL;
    std::shared_ptr<CommJob> j;
    try { j = std::make_shared<CommJob>(); } catch (...) { return ENOMEM; }
    j->want_id = true;
    const int rc = run_comm_job(j, comm_timeout_s());
    if (rc == 0) memcpy(id, &j->id, sizeof(j->id));
    return rc;
}

extern "C" rmgr_int32_t rmgr_ssim_hip_comm_init(rmgr_ssim_hip_Context* c, const unsigned char id[RMGR_SSIM_HIP_COMM_ID_BYTES],
                                                rmgr_int32_t rankCount, rmgr_int32_t rank) RMGR_NOEXCEPT
{
    if (!c || !id || rankCount < 1 || rank < 0 || rank >= rankCount || c->comm) return EINVAL;
    std::shared_ptr<CommJob> j;
    try { j = std::make_shared<CommJob>(); } catch (...) { return ENOMEM; }
    j->device = c->device;
    j->rank_count = rankCount;
    j->rank = rank;
    if (const char* e = getenv("RMGR_SSIM_HIP_COMM_BLOCKING")) j->nonblocking_ok = atoi(e) == 0;
    memcpy(&j->id, id, sizeof(j->id));
    const int rc = run_comm_job(j, comm_timeout_s());
    if (rc) return rc;
    c->comm = j->comm;
    c->comm_nonblocking = j->nonblocking;
    c->comm_ranks = 0;
    Rccl* r = rccl();
    int n = 0;
    if (r && r->CommCount(c->comm, &n) == ncclSuccess) c->comm_ranks = n;
    return 0;
}

extern "C" rmgr_int32_t rmgr_ssim_hip_comm_rank_count(const rmgr_ssim_hip_Context* c, rmgr_int32_t* rankCount) RMGR_NOEXCEPT
{
    if (!c || !rankCount) return EINVAL;
    *rankCount = c->comm ? c->comm_ranks : 0;      // what RCCL itself reports for the communicator (ncclCommCount), 0 without one
    return 0;
}

extern "C" rmgr_int32_t rmgr_ssim_hip_comm_allreduce_sums(rmgr_ssim_hip_Context* c, double* sumsDevice, rmgr_uint32_t count) RMGR_NOEXCEPT
{
    if (!c || !c->comm || (count && !sumsDevice)) return EINVAL;
    if (count == 0) return 0;
    Rccl* r = rccl();
    if (!r) return ENOSYS;
    USE_DEVICE(c);
    rmgr_ssim_hip_Context_::Collective k;
    k.begin = comm_take_event(c); k.end = comm_take_event(c); k.started = false;
    if (!k.begin || !k.end) { if (k.begin) c->spare_events.push_back(k.begin); return ENOMEM; }
    if (hipEventRecord(k.begin, c->stream) != hipSuccess) {
        (void)hipGetLastError();
        c->spare_events.push_back(k.begin); c->spare_events.push_back(k.end);
        return ECHILD;
    }
    const int rc = comm_wait_ready(r, c, r->AllReduce(sumsDevice, sumsDevice, count, ncclFloat64, ncclSum, c->comm, c->stream));
    if (rc == ETIMEDOUT) comm_abort(r, c);         // the enqueue itself never completed: the communicator is gone
    if (rc == 0 && hipEventRecord(k.end, c->stream) == hipSuccess) {
        c->collectives.push_back(k);               // rmgr_ssim_hip_synchronize bounds its wait for THIS collective (comm_bounded_sync)
        while (c->collectives.size() > 64) {       // a caller that never synchronises: the oldest have long completed or will be caught by the next
            if (hipEventQuery(c->collectives.front().end) != hipSuccess) { (void)hipGetLastError(); break; }
            c->spare_events.push_back(c->collectives.front().begin); c->spare_events.push_back(c->collectives.front().end);
            c->collectives.pop_front();
        }
    } else {
        (void)hipGetLastError();
        c->spare_events.push_back(k.begin); c->spare_events.push_back(k.end);
    }
    return rc;
}

extern "C" rmgr_int32_t rmgr_ssim_hip_comm_destroy(rmgr_ssim_hip_Context* c) RMGR_NOEXCEPT
{
    if (!c) return EINVAL;
    if (!c->comm) return 0;
    Rccl* r = rccl();
    if (!r) { c->comm = NULL; return ENOSYS; }
    USE_DEVICE(c);
    int rc = 0;
    if (!c->collectives.empty()) {                 // queued all-reduces first, with their deadline: a stuck one aborts the communicator
        rc = comm_bounded_sync(c);
        if (!c->comm) return rc;
    }
    if (c->comm_nonblocking && r->CommFinalize) {
        // ncclCommFinalize is the asynchronous half of the teardown; ncclCommDestroy then only frees
        rc = comm_wait_ready(r, c, r->CommFinalize(c->comm));
        if (rc == ETIMEDOUT) { comm_abort(r, c); return rc; }
    }
    const int rd = map_nccl(r->CommDestroy(c->comm));
    c->comm = NULL;
    c->comm_nonblocking = false;
    c->comm_ranks = 0;
    return rc ? rc : rd;
}

extern "C" const char* rmgr_ssim_hip_comm_describe(void) RMGR_NOEXCEPT
{
    static char text[384];
    static std::mutex m;
    std::lock_guard<std::mutex> lk(m);
    Rccl* r = rccl();
    if (!r) snprintf(text, sizeof(text), "rccl: not loadable (%s)", dlerror() ? "dlopen failed" : "no usable librccl");
    else snprintf(text, sizeof(text), "rccl %d.%d.%d from %s; non-blocking init %s; deadline %.1f s", r->version / 10000, (r->version / 100) % 100, r->version % 100,
                  r->path[0] ? r->path : "?", (r->CommInitRankConfig && r->CommGetAsyncError && r->CommAbort) ? "available" : "unavailable", comm_timeout_s());
    return text;
}
