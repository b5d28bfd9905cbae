// Test-only stand-in for the eight RCCL entry points legged_gym_dev_amd/csrc/comm_api.cpp resolves (selected with LG_RCCL_LIB).
// The ranks of a communicator are THREADS OF ONE PROCESS sharing one device, so every rank can read its peers' buffers directly.
//
// What it keeps of RCCL: a collective is work enqueued on the stream the caller hands in -- nothing here synchronises a stream or the
// device, so a caller that forgets a stream wait reads stale data exactly as it would over RCCL.  What it adds: the ranks compare their
// calls and a host rendezvous has a time limit, so a mismatch or a missing rank is an error code with a message instead of a hang.
//
// One group (ncclGroupStart .. ncclGroupEnd, or a lone call) on rank r with stream s:
//   1. s waits for r's previous copy-back (the scratch is reused), r records READY on s          -- r's inputs are complete at READY
//   2. host rendezvous: every rank has posted its calls; they are compared (operation, count, root, number of calls)
//   3. s waits for every peer's READY;  per call a kernel writes scratch_r[i] = buf_0[i] + buf_1[i] + ... in rank order
//      (broadcast: an asynchronous copy root's buffer -> scratch_r)
//   4. r records READ on s;  host rendezvous;  s waits for every peer's READ                      -- nobody still reads r's buffers
//   5. the optional delay kernel, then per call an asynchronous copy scratch_r -> buf_r
// Sums run in rank order on every rank: all ranks receive the same bits.  No device code waits on memory; ranks meet on the host only.
// ncclCommInitRank only registers the rank (it does not wait for the peers): the first collective's rendezvous is where they meet.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace {

typedef struct { char internal[128]; } nccl_uid;
const int kMaxRanks = 8, kMaxCalls = 16;
const size_t kScratchFloats = (size_t)1 << 20;             // per rank and group, allocated once in ncclCommInitRank
const int kFloat32 = 7, kSum = 0;
const int kErrInternal = 3, kErrArgument = 4, kErrUsage = 5;   // ncclInternalError, ncclInvalidArgument, ncclInvalidUsage
enum { OP_ALLREDUCE = 1, OP_BROADCAST = 2 };

std::atomic<int> g_delay_us{0};
std::atomic<int> g_timeout_ms{30000};
thread_local std::string t_msg;

int fail(int code, const std::string &m) { t_msg = "standin: " + m; return code; }
const char *op_name(int op) { return op == OP_ALLREDUCE ? "ncclAllReduce" : op == OP_BROADCAST ? "ncclBroadcast" : "nothing"; }

struct Call { int op; size_t count; int root; const float *send; float *recv; };
struct Post { int n; Call c[kMaxCalls]; };
struct LogEntry { int64_t op, count, grouped, group; };

struct Group;
struct Comm {
    Group *g; int rank;
    float *scratch;
    hipEvent_t ready, read, copied;
    int64_t groups_issued;
    std::vector<LogEntry> log;
};

struct Group {
    std::mutex m;
    std::condition_variable cv;
    int nranks = 0, joined = 0, arrived = 0;
    uint64_t generation = 0;
    bool broken = false;
    std::string why;
    bool here[kMaxRanks] = {};
    Comm *rank[kMaxRanks] = {};
    Post post[kMaxRanks];
};

std::mutex g_mutex;
std::map<std::string, Group *> g_groups;
std::atomic<uint64_t> g_uid_counter{0};

std::string describe(const Post &p) {
    std::string s = std::to_string(p.n) + " call(s):";
    char b[96];
    for (int k = 0; k < p.n; ++k) {
        snprintf(b, sizeof b, " %s(count=%zu, root=%d)", op_name(p.c[k].op), p.c[k].count, p.c[k].root);
        s += b;
    }
    return s;
}

// All ranks of the group meet here, or every waiting rank gives up after the time limit and the group stays broken.
int rendezvous(Group *g, int me, const char *what) {
    std::unique_lock<std::mutex> lk(g->m);
    if (g->broken) return fail(kErrInternal, "communicator is broken: " + g->why);
    const uint64_t gen = g->generation;
    g->here[me] = true;
    if (++g->arrived == g->nranks) {
        g->arrived = 0;
        for (int r = 0; r < g->nranks; ++r) g->here[r] = false;
        ++g->generation;
        g->cv.notify_all();
        return 0;
    }
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(g_timeout_ms.load());
    while (g->generation == gen && !g->broken)
        if (g->cv.wait_until(lk, deadline) == std::cv_status::timeout && g->generation == gen && !g->broken) {
            std::string missing;
            for (int r = 0; r < g->nranks; ++r)
                if (!g->here[r]) missing += (missing.empty() ? "" : ", ") + std::to_string(r);
            g->broken = true;
            g->why = "rank " + missing + " did not arrive at " + what + " within " + std::to_string(g_timeout_ms.load()) +
                     " ms (rank " + std::to_string(me) + " waited)";
            g->cv.notify_all();
        }
    if (g->generation == gen) return fail(kErrInternal, g->why);
    return 0;
}

struct SumArgs { const float *src[kMaxRanks]; };
__global__ void k_sum(float *out, SumArgs a, int nranks, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float s = a.src[0][i];
        for (int r = 1; r < nranks; ++r) s += a.src[r][i];
        out[i] = s;
    }
}
// One wave that reads the wall clock until `ticks` have passed, at most `cap` times; touches no memory.
__global__ void k_delay(long long ticks, int cap) {
    const long long t0 = wall_clock64();
    for (int it = 0; it < cap && wall_clock64() - t0 < ticks; ++it) {}
}

bool hip_ok(hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    fail(kErrInternal, std::string(what) + ": " + hipGetErrorString(e));
    return false;
}

int issue(Comm *c, const Post &mine, hipStream_t s, bool grouped) {
    Group *g = c->g;
    const int me = c->rank, W = g->nranks;
    size_t total = 0;
    for (int k = 0; k < mine.n; ++k) total += mine.c[k].count;
    if (total > kScratchFloats)
        return fail(kErrArgument, "a group of " + std::to_string(total) + " floats is above the fixed scratch capacity of " + std::to_string(kScratchFloats));
    char what[96];
    snprintf(what, sizeof what, "%s(count=%zu)%s", op_name(mine.c[0].op), mine.c[0].count, mine.n > 1 ? " [first of a group]" : "");
    if (!hip_ok(hipStreamWaitEvent(s, c->copied, 0), "hipStreamWaitEvent") || !hip_ok(hipEventRecord(c->ready, s), "hipEventRecord")) return kErrInternal;
    {
        std::lock_guard<std::mutex> lk(g->m);
        g->post[me] = mine;
    }
    if (int rc = rendezvous(g, me, what)) return rc;
    Post peer[kMaxRanks];
    hipEvent_t ready[kMaxRanks], read[kMaxRanks];
    {
        std::lock_guard<std::mutex> lk(g->m);
        for (int r = 0; r < W; ++r) { peer[r] = g->post[r]; ready[r] = g->rank[r]->ready; read[r] = g->rank[r]->read; }
    }
    for (int b = 1; b < W; ++b) {                             // every rank reads the same posts: a disagreement is an error on all of them
        bool eq = peer[0].n == peer[b].n;
        for (int k = 0; eq && k < peer[0].n; ++k)
            eq = peer[0].c[k].op == peer[b].c[k].op && peer[0].c[k].count == peer[b].c[k].count && peer[0].c[k].root == peer[b].c[k].root;
        if (!eq) return fail(kErrUsage, "the ranks disagree: rank 0 issued " + describe(peer[0]) + " but rank " + std::to_string(b) +
                                        " issued " + describe(peer[b]));
    }
    for (int r = 0; r < W; ++r)
        if (r != me && !hip_ok(hipStreamWaitEvent(s, ready[r], 0), "hipStreamWaitEvent")) return kErrInternal;
    size_t off = 0;
    for (int k = 0; k < mine.n; ++k) {
        const Call &q = mine.c[k];
        if (q.op == OP_ALLREDUCE) {
            SumArgs a;
            for (int r = 0; r < kMaxRanks; ++r) a.src[r] = r < W ? peer[r].c[k].send : nullptr;
            const unsigned blocks = (unsigned)((q.count + 255) / 256 < 1024 ? (q.count + 255) / 256 : 1024);
            hipLaunchKernelGGL(k_sum, dim3(blocks), dim3(256), 0, s, c->scratch + off, a, W, q.count);
            if (!hip_ok(hipGetLastError(), "k_sum launch")) return kErrInternal;
        } else if (!hip_ok(hipMemcpyAsync(c->scratch + off, peer[q.root].c[k].send, q.count * sizeof(float), hipMemcpyDeviceToDevice, s), "hipMemcpyAsync"))
            return kErrInternal;
        off += q.count;
    }
    if (!hip_ok(hipEventRecord(c->read, s), "hipEventRecord")) return kErrInternal;
    if (int rc = rendezvous(g, me, what)) return rc;
    for (int r = 0; r < W; ++r)
        if (r != me && !hip_ok(hipStreamWaitEvent(s, read[r], 0), "hipStreamWaitEvent")) return kErrInternal;
    if (const int us = g_delay_us.load()) {
        int khz = 0, dev = 0;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;
        hipLaunchKernelGGL(k_delay, dim3(1), dim3(64), 0, s, (long long)us * khz / 1000, us * 200 + 1000);
        if (!hip_ok(hipGetLastError(), "k_delay launch")) return kErrInternal;
    }
    off = 0;
    for (int k = 0; k < mine.n; ++k) {
        if (!hip_ok(hipMemcpyAsync(mine.c[k].recv, c->scratch + off, mine.c[k].count * sizeof(float), hipMemcpyDeviceToDevice, s), "hipMemcpyAsync")) return kErrInternal;
        off += mine.c[k].count;
    }
    if (!hip_ok(hipEventRecord(c->copied, s), "hipEventRecord")) return kErrInternal;
    {
        std::lock_guard<std::mutex> lk(g->m);
        for (int k = 0; k < mine.n; ++k) c->log.push_back({mine.c[k].op, (int64_t)mine.c[k].count, grouped ? 1 : 0, c->groups_issued});
        ++c->groups_issued;
    }
    return 0;
}

// ncclGroupStart .. ncclGroupEnd of the calling thread
thread_local int t_depth = 0;
thread_local Post t_queue;
thread_local Comm *t_comm = nullptr;
thread_local hipStream_t t_stream = nullptr;
thread_local int t_queue_rc = 0;

int enqueue(int op, const void *send, void *recv, size_t count, int dtype, int redop, int root, void *comm, hipStream_t s) {
    Comm *c = (Comm *)comm;
    if (!c || !send || !recv) return fail(kErrArgument, "null communicator or buffer");
    if (dtype != kFloat32) return fail(kErrArgument, "only float32 is carried (datatype " + std::to_string(dtype) + ")");
    if (op == OP_ALLREDUCE && redop != kSum) return fail(kErrArgument, "only the sum is carried (reduction " + std::to_string(redop) + ")");
    if (op == OP_BROADCAST && (root < 0 || root >= c->g->nranks)) return fail(kErrArgument, "root " + std::to_string(root) + " is no rank");
    if (count == 0) return 0;
    const Call q = {op, count, op == OP_BROADCAST ? root : -1, (const float *)send, (float *)recv};
    if (t_depth == 0) {
        Post p;
        p.n = 1; p.c[0] = q;
        return issue(c, p, s, false);
    }
    if (t_queue.n > 0 && (c != t_comm || s != t_stream)) return t_queue_rc = fail(kErrUsage, "a group carries one communicator on one stream");
    if (t_queue.n == kMaxCalls) return t_queue_rc = fail(kErrUsage, "more than " + std::to_string(kMaxCalls) + " calls in a group");
    t_comm = c; t_stream = s;
    t_queue.c[t_queue.n++] = q;
    return 0;
}

}  // namespace

extern "C" {

int ncclGetUniqueId(nccl_uid *out) {
    if (!out) return fail(kErrArgument, "null id");
    memset(out, 0, sizeof(*out));
    const uint64_t n = ++g_uid_counter;
    const uint64_t t = (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count();
    memcpy(out->internal, "standin", 8);
    memcpy(out->internal + 8, &n, 8);
    memcpy(out->internal + 16, &t, 8);
    return 0;
}

int ncclCommInitRank(void **comm, int nranks, nccl_uid id, int rank) {
    if (!comm) return fail(kErrArgument, "null communicator");
    if (nranks < 2 || nranks > kMaxRanks) return fail(kErrArgument, "2 to 8 ranks are carried, not " + std::to_string(nranks));
    if (rank < 0 || rank >= nranks) return fail(kErrArgument, "rank " + std::to_string(rank) + " of " + std::to_string(nranks));
    Comm *c = new Comm();
    c->rank = rank; c->groups_issued = 0; c->scratch = nullptr;
    if (!hip_ok(hipMalloc((void **)&c->scratch, kScratchFloats * sizeof(float)), "hipMalloc") ||
        !hip_ok(hipEventCreateWithFlags(&c->ready, hipEventDisableTiming), "hipEventCreate") ||
        !hip_ok(hipEventCreateWithFlags(&c->read, hipEventDisableTiming), "hipEventCreate") ||
        !hip_ok(hipEventCreateWithFlags(&c->copied, hipEventDisableTiming), "hipEventCreate")) { delete c; return kErrInternal; }
    std::lock_guard<std::mutex> lk(g_mutex);
    Group *&g = g_groups[std::string(id.internal, sizeof(id.internal))];
    if (!g) { g = new Group(); g->nranks = nranks; }
    std::lock_guard<std::mutex> lk2(g->m);
    if (g->nranks != nranks || g->rank[rank]) {
        (void)hipFree(c->scratch);
        delete c;
        return fail(kErrUsage, "rank " + std::to_string(rank) + " of " + std::to_string(nranks) + " does not fit the communicator of this id (" +
                                   std::to_string(g->nranks) + " ranks" + (g->nranks == nranks ? ", rank taken)" : ")"));
    }
    c->g = g;
    g->rank[rank] = c;
    ++g->joined;
    *comm = c;
    return 0;
}

int ncclCommDestroy(void *comm) {
    Comm *c = (Comm *)comm;
    if (!c) return 0;
    std::lock_guard<std::mutex> lk(g_mutex);
    Group *g = c->g;
    bool last;
    {
        std::lock_guard<std::mutex> lk2(g->m);
        g->rank[c->rank] = nullptr;
        last = --g->joined == 0;
        if (!last && !g->broken) { g->broken = true; g->why = "rank " + std::to_string(c->rank) + " destroyed its communicator"; g->cv.notify_all(); }
    }
    if (last) {
        for (auto it = g_groups.begin(); it != g_groups.end(); ++it)
            if (it->second == g) { g_groups.erase(it); break; }
        delete g;
    }
    (void)hipFree(c->scratch);                                 // synchronises the device: nothing enqueued still uses it
    (void)hipEventDestroy(c->ready); (void)hipEventDestroy(c->read); (void)hipEventDestroy(c->copied);
    delete c;
    return 0;
}

int ncclAllReduce(const void *send, void *recv, size_t count, int dtype, int op, void *comm, hipStream_t s) {
    return enqueue(OP_ALLREDUCE, send, recv, count, dtype, op, -1, comm, s);
}
int ncclBroadcast(const void *send, void *recv, size_t count, int dtype, int root, void *comm, hipStream_t s) {
    return enqueue(OP_BROADCAST, send, recv, count, dtype, kSum, root, comm, s);
}
int ncclGroupStart(void) {
    if (t_depth++ == 0) { t_queue.n = 0; t_queue_rc = 0; t_comm = nullptr; t_stream = nullptr; }
    return 0;
}
int ncclGroupEnd(void) {
    if (t_depth == 0) return fail(kErrUsage, "ncclGroupEnd without ncclGroupStart");
    if (--t_depth > 0) return 0;
    if (t_queue_rc) return t_queue_rc;                          // t_msg still holds the reason
    if (t_queue.n == 0) return 0;
    return issue(t_comm, t_queue, t_stream, true);
}
const char *ncclGetErrorString(int rc) {
    if (rc == 0) return "no error";
    return t_msg.empty() ? "standin: error" : t_msg.c_str();
}

// ---- test controls (not part of RCCL)
// Microseconds the delay kernel holds every copy-back (0 .. 5000; 0 = no kernel).  Process-wide.
int standin_set_delay_us(int us) {
    if (us < 0 || us > 5000) return fail(kErrArgument, "delay outside 0 .. 5000 us");
    g_delay_us = us;
    return 0;
}
// Time limit of a host rendezvous in ms (default 30000); shortened only by the test of a rank that never arrives.
int standin_set_timeout_ms(int ms) {
    if (ms < 1 || ms > 30000) return fail(kErrArgument, "time limit outside 1 .. 30000 ms");
    g_timeout_ms = ms;
    return 0;
}
// The calls rank `rank` of the communicator with this id has issued since the last reset, oldest first: per call four int64 =
// (operation: 1 all-reduce, 2 broadcast; count; 1 inside ncclGroupStart/End, else 0; ordinal of the group that carried it).
// Writes at most `cap` calls and returns how many there are, -1 for an unknown communicator.  reset != 0 empties the log.
int64_t standin_call_log(const void *id, int rank, int64_t *out, int64_t cap, int reset) {
    std::lock_guard<std::mutex> lk(g_mutex);
    auto it = g_groups.find(std::string((const char *)id, sizeof(nccl_uid)));
    if (it == g_groups.end() || rank < 0 || rank >= it->second->nranks) return -1;
    std::lock_guard<std::mutex> lk2(it->second->m);
    Comm *c = it->second->rank[rank];
    if (!c) return -1;
    const int64_t n = (int64_t)c->log.size();
    for (int64_t k = 0; k < n && k < cap && out; ++k) {
        out[4 * k] = c->log[k].op; out[4 * k + 1] = c->log[k].count; out[4 * k + 2] = c->log[k].grouped; out[4 * k + 3] = c->log[k].group;
    }
    if (reset) { c->log.clear(); c->groups_issued = 0; }
    return n;
}

}  // extern "C"
