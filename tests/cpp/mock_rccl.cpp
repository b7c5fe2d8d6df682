// mock_rccl.cpp -- a stand-in for RCCL that lets the N-device group of csrc/drt_group.cpp run on one GPU (DRT_RCCL_LIB=<this .so>,
// DRT_GROUP_SHARE_DEVICE=1).  It exports the seven entry points drt_group.cpp binds, with NCCL's semantics for what the group uses
// (grouped point-to-point), and moves the bytes with hipMemcpyAsync on the receiver's stream.  Built by the tests:
//   g++ -std=c++17 -shared -fPIC -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include mock_rccl.cpp -L/opt/rocm/lib -lamdhip64
//
// Semantics:
//  * ncclCommInitAll accepts any device list, duplicates included; rank i is position i.
//  * ncclGroupStart / ncclGroupEnd nest by depth.  ncclSend / ncclRecv inside a group only queue the operation; outside one they
//    return ncclInvalidUsage (and count a violation: the product never does that).
//  * A Send or Recv that fails inside a group poisons it, as in NCCL: the outermost ncclGroupEnd then returns that error and drops
//    everything queued, executing nothing.
//  * At the outermost ncclGroupEnd every Send (rank s -> peer p) is matched with the Recv (rank p <- peer s) of the same
//    communicator set, in issue order per pair.  An unmatched operation, a count mismatch or a transfer that does not fit in its
//    allocation is a violation: the call returns ncclInvalidUsage at once, drops the queue and moves nothing -- it never waits.
//  * A matched pair: an event recorded on the sender's stream, the receiver's stream waits for it, hipMemcpyAsync on the receiver's
//    stream, an event recorded there that the sender's stream waits for (its buffer is not reused before the copy).  Every event
//    is recorded before the wait that names it is issued, in host order: streams of one process share hardware queues, and a
//    wait queued ahead of its record on the same queue would block that queue.
//  * Events are kept until their communicator is destroyed (the group synchronises its streams before that).
//
// Control, for the tests (ctypes on the same path): mock_rccl_reset, mock_rccl_fail (fail the k-th call of a kind with
// ncclSystemError; a failed operation is not queued), the call log, open depth, queued operations, violations.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <deque>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <tuple>
#include <vector>

namespace {

enum Result { ncclSuccess = 0, ncclUnhandledCudaError = 1, ncclSystemError = 2, ncclInternalError = 3, ncclInvalidArgument = 4, ncclInvalidUsage = 5 };
// kinds of calls, as the log and mock_rccl_fail name them
enum Kind { kInitAll = 0, kSend = 1, kRecv = 2, kGroupEnd = 3, kGroupStart = 4, kDestroy = 5, kKinds = 6 };
constexpr int kFloat32 = 7;                    // ncclFloat32

struct Comm {
    int clique, rank, nranks, device;
    std::vector<hipEvent_t> events;
};
struct Op {
    Kind kind;
    Comm *comm;
    int peer;
    void *buf;
    size_t count;
    hipStream_t stream;
};
struct LogEntry {
    int kind, rank, peer;
    uint64_t count;
    void *stream;
    int result;
};

std::mutex mu;
int depth = 0;
int group_error = ncclSuccess;                 // first failure of a Send / Recv inside the open group
std::vector<Op> queued;
std::vector<LogEntry> call_log;
std::set<Comm *> live;
uint64_t calls[kKinds] = {}, fail_at[kKinds] = {};
uint64_t violations = 0, pairs_moved = 0;
std::string last_violation;
int next_clique = 0;

int violation(int rc, const std::string &what) {
    violations++;
    last_violation = what;
    return rc;
}

int logged(Kind kind, const Comm *comm, int peer, uint64_t count, void *stream, int result) {
    call_log.push_back(LogEntry{ kind, comm ? comm->rank : -1, peer, count, stream, result });
    return result;
}

bool injected(Kind kind) { return ++calls[kind] == fail_at[kind]; }

// the allocation that holds [p, p + bytes), or false
bool inside_allocation(const void *p, size_t bytes) {
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(p)) != hipSuccess || !base) return false;
    const uintptr_t b = reinterpret_cast<uintptr_t>(base), q = reinterpret_cast<uintptr_t>(p);
    return q >= b && q - b <= size && bytes <= size - (q - b);
}

int enqueue(Kind kind, void *buf, size_t count, int datatype, int peer, void *comm_, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(mu);
    Comm *comm = live.count(static_cast<Comm *>(comm_)) ? static_cast<Comm *>(comm_) : nullptr;
    int rc = ncclSuccess;
    if (injected(kind)) rc = ncclSystemError;
    else if (!comm || peer < 0 || peer >= comm->nranks || datatype != kFloat32 || (count && !buf))
        rc = violation(ncclInvalidArgument, kind == kSend ? "ncclSend: bad argument" : "ncclRecv: bad argument");
    else if (depth == 0)
        rc = violation(ncclInvalidUsage, kind == kSend ? "ncclSend outside a group" : "ncclRecv outside a group");
    if (rc != ncclSuccess) {
        if (depth > 0 && group_error == ncclSuccess) group_error = rc;
        return logged(kind, comm, peer, count, stream, rc);
    }
    queued.push_back(Op{ kind, comm, peer, buf, count, stream });
    return logged(kind, comm, peer, count, stream, ncclSuccess);
}

// the matched pairs of the queue in execution order, or a violation
int match(std::vector<std::pair<const Op *, const Op *>> &pairs) {
    std::map<std::tuple<int, int, int>, std::deque<const Op *>> recvs;      // (clique, sender, receiver) -> receives in issue order
    for (const Op &op : queued)
        if (op.kind == kRecv) recvs[std::make_tuple(op.comm->clique, op.peer, op.comm->rank)].push_back(&op);
    for (const Op &op : queued) {
        if (op.kind != kSend) continue;
        auto it = recvs.find(std::make_tuple(op.comm->clique, op.comm->rank, op.peer));
        if (it == recvs.end() || it->second.empty())
            return violation(ncclInvalidUsage, "ncclSend from rank " + std::to_string(op.comm->rank) + " to " + std::to_string(op.peer) + " has no matching ncclRecv");
        const Op *r = it->second.front();
        it->second.pop_front();
        if (r->count != op.count)
            return violation(ncclInvalidUsage, "count mismatch: rank " + std::to_string(op.comm->rank) + " sends " + std::to_string(op.count) +
                                                   ", rank " + std::to_string(r->comm->rank) + " receives " + std::to_string(r->count));
        const size_t bytes = op.count * sizeof(float);
        if (bytes && (!inside_allocation(op.buf, bytes) || !inside_allocation(r->buf, bytes)))
            return violation(ncclInvalidUsage, "a transfer of " + std::to_string(bytes) + " bytes from rank " + std::to_string(op.comm->rank) +
                                                   " does not fit in its source or destination allocation");
        pairs.emplace_back(&op, r);
    }
    for (auto &kv : recvs)
        if (!kv.second.empty())
            return violation(ncclInvalidUsage, "ncclRecv on rank " + std::to_string(std::get<2>(kv.first)) + " from " + std::to_string(std::get<1>(kv.first)) +
                                                   " has no matching ncclSend");
    return ncclSuccess;
}

int execute(const std::vector<std::pair<const Op *, const Op *>> &pairs) {
    int current = 0;
    if (hipGetDevice(&current) != hipSuccess) return ncclUnhandledCudaError;
    int rc = ncclSuccess;
    auto ok = [&](hipError_t e) { if (e != hipSuccess && rc == ncclSuccess) rc = ncclUnhandledCudaError; return rc == ncclSuccess; };
    for (const auto &p : pairs) {
        const Op &s = *p.first, &r = *p.second;
        if (s.count == 0) continue;
        hipEvent_t sent = nullptr, copied = nullptr;
        if (!ok(hipSetDevice(s.comm->device)) || !ok(hipEventCreateWithFlags(&sent, hipEventDisableTiming))) break;
        s.comm->events.push_back(sent);
        if (!ok(hipEventRecord(sent, s.stream))) break;
        if (!ok(hipSetDevice(r.comm->device)) || !ok(hipStreamWaitEvent(r.stream, sent, 0)) ||
            !ok(hipMemcpyAsync(r.buf, s.buf, s.count * sizeof(float), hipMemcpyDeviceToDevice, r.stream)) ||
            !ok(hipEventCreateWithFlags(&copied, hipEventDisableTiming)))
            break;
        r.comm->events.push_back(copied);
        if (!ok(hipEventRecord(copied, r.stream)) || !ok(hipSetDevice(s.comm->device)) || !ok(hipStreamWaitEvent(s.stream, copied, 0))) break;
        pairs_moved++;
    }
    (void)hipSetDevice(current);
    return rc;
}

}  // namespace

extern "C" {

int ncclCommInitAll(void **comms, int ndev, const int *devlist) {
    std::lock_guard<std::mutex> lock(mu);
    if (injected(kInitAll)) return logged(kInitAll, nullptr, -1, (uint64_t)ndev, nullptr, ncclSystemError);
    if (!comms || ndev < 1) return logged(kInitAll, nullptr, -1, (uint64_t)ndev, nullptr, violation(ncclInvalidArgument, "ncclCommInitAll: bad argument"));
    const int clique = next_clique++;
    for (int i = 0; i < ndev; i++) {
        Comm *c = new Comm{ clique, i, ndev, devlist ? devlist[i] : i, {} };
        live.insert(c);
        comms[i] = c;
    }
    return logged(kInitAll, nullptr, -1, (uint64_t)ndev, nullptr, ncclSuccess);
}

int ncclCommDestroy(void *comm_) {
    std::lock_guard<std::mutex> lock(mu);
    calls[kDestroy]++;
    Comm *comm = static_cast<Comm *>(comm_);
    if (!live.count(comm)) return logged(kDestroy, nullptr, -1, 0, nullptr, violation(ncclInvalidArgument, "ncclCommDestroy of an unknown communicator"));
    for (const Op &op : queued)
        if (op.comm == comm) return logged(kDestroy, comm, -1, 0, nullptr, violation(ncclInvalidUsage, "ncclCommDestroy with operations queued"));
    int current = 0;
    const bool restore = hipGetDevice(&current) == hipSuccess;
    (void)hipSetDevice(comm->device);
    for (hipEvent_t e : comm->events) (void)hipEventDestroy(e);
    if (restore) (void)hipSetDevice(current);
    live.erase(comm);
    logged(kDestroy, comm, -1, 0, nullptr, ncclSuccess);
    delete comm;
    return ncclSuccess;
}

int ncclGroupStart() {
    std::lock_guard<std::mutex> lock(mu);
    calls[kGroupStart]++;
    depth++;
    return logged(kGroupStart, nullptr, -1, 0, nullptr, ncclSuccess);
}

int ncclGroupEnd() {
    std::lock_guard<std::mutex> lock(mu);
    if (depth == 0) {
        calls[kGroupEnd]++;
        return logged(kGroupEnd, nullptr, -1, 0, nullptr, violation(ncclInvalidUsage, "ncclGroupEnd without ncclGroupStart"));
    }
    if (injected(kGroupEnd) && group_error == ncclSuccess) group_error = ncclSystemError;
    if (--depth > 0) return logged(kGroupEnd, nullptr, -1, 0, nullptr, group_error);
    int rc = group_error;
    group_error = ncclSuccess;
    if (rc == ncclSuccess) {
        std::vector<std::pair<const Op *, const Op *>> pairs;
        rc = match(pairs);
        if (rc == ncclSuccess) rc = execute(pairs);
    }
    const uint64_t n = queued.size();
    queued.clear();
    return logged(kGroupEnd, nullptr, -1, n, nullptr, rc);
}

int ncclSend(const void *buf, size_t count, int datatype, int peer, void *comm, hipStream_t stream) {
    return enqueue(kSend, const_cast<void *>(buf), count, datatype, peer, comm, stream);
}

int ncclRecv(void *buf, size_t count, int datatype, int peer, void *comm, hipStream_t stream) {
    return enqueue(kRecv, buf, count, datatype, peer, comm, stream);
}

const char *ncclGetErrorString(int result) {
    switch (result) {
    case ncclSuccess: return "no error";
    case ncclUnhandledCudaError: return "unhandled HIP error (mock RCCL)";
    case ncclSystemError: return "unhandled system error (mock RCCL, injected)";
    case ncclInternalError: return "internal error (mock RCCL)";
    case ncclInvalidArgument: return "invalid argument (mock RCCL)";
    case ncclInvalidUsage: return "invalid usage (mock RCCL)";
    default: return "unknown result (mock RCCL)";
    }
}

// ---- control, for the tests ----
// Forget the log, the call counts, armed failures and violations; an open group and its queue are dropped.  Live communicators stay.
void mock_rccl_reset() {
    std::lock_guard<std::mutex> lock(mu);
    call_log.clear();
    for (int k = 0; k < kKinds; k++) calls[k] = fail_at[k] = 0;
    violations = pairs_moved = 0;
    last_violation.clear();
    depth = 0;
    group_error = ncclSuccess;
    queued.clear();
}

// The k-th call (1-based, counted from the last reset) of `kind` (kInitAll, kSend, kRecv, kGroupEnd) fails with ncclSystemError;
// k = 0 disarms.  Returns -1 for a kind that cannot be failed.
int mock_rccl_fail(int kind, uint64_t k) {
    std::lock_guard<std::mutex> lock(mu);
    if (kind != kInitAll && kind != kSend && kind != kRecv && kind != kGroupEnd) return -1;
    fail_at[kind] = k ? calls[kind] + k : 0;
    return 0;
}

int mock_rccl_depth() { std::lock_guard<std::mutex> lock(mu); return depth; }
uint64_t mock_rccl_queued() { std::lock_guard<std::mutex> lock(mu); return queued.size(); }
uint64_t mock_rccl_violations() { std::lock_guard<std::mutex> lock(mu); return violations; }
uint64_t mock_rccl_pairs_moved() { std::lock_guard<std::mutex> lock(mu); return pairs_moved; }
int mock_rccl_live_comms() { std::lock_guard<std::mutex> lock(mu); return (int)live.size(); }

// Copies the last violation's description into buf (NUL-terminated); returns its length.
int mock_rccl_last_violation(char *buf, size_t cap) {
    std::lock_guard<std::mutex> lock(mu);
    if (buf && cap) std::snprintf(buf, cap, "%s", last_violation.c_str());
    return (int)last_violation.size();
}

uint64_t mock_rccl_log_size() { std::lock_guard<std::mutex> lock(mu); return call_log.size(); }

// Entry i of the call log: kind (see mock_rccl_fail; 4 ncclGroupStart, 5 ncclCommDestroy), communicator rank (-1: none), peer,
// count (elements; ncclCommInitAll: ndev; outermost ncclGroupEnd: operations it consumed), stream, result.  -1 when out of range.
int mock_rccl_log_entry(uint64_t i, int *kind, int *rank, int *peer, uint64_t *count, void **stream, int *result) {
    std::lock_guard<std::mutex> lock(mu);
    if (i >= call_log.size()) return -1;
    const LogEntry &e = call_log[i];
    if (kind) *kind = e.kind;
    if (rank) *rank = e.rank;
    if (peer) *peer = e.peer;
    if (count) *count = e.count;
    if (stream) *stream = e.stream;
    if (result) *result = e.result;
    return 0;
}

}  // extern "C"
