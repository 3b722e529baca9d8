// Test double of librccl.so.1 for tests/test_film_reduce_ranks.py: the eight entry points hk_comm.cpp resolves (the Rccl struct), with
// the prototypes of <rccl/rccl.h>, so that hk_film_reduce runs with 2 or 3 ranks on ONE device (real RCCL refuses two ranks per GPU).
// Ranks are processes that share a file under $FAKE_RCCL_DIR (mmap MAP_SHARED; the unique id names the file, every rank resolves the
// name in its own $FAKE_RCCL_DIR, so the directory may be of any length); the library finds the double first because the test
// puts its directory at the head of LD_LIBRARY_PATH (libhikari_mi355x.so carries a RUNPATH).  Host-only C++ against the HIP runtime.
//
// ncclReduce is asynchronous and ordered on its stream like the real one: device -> pinned copy, a host function that exchanges through
// the shared file (rank-order sum in the element type, on the root), and on the root a pinned -> device copy into recvbuff.  The host
// function makes no HIP call.  Every wait gives up after FAKE_RCCL_TIMEOUT_S (60) seconds: the error is logged and flagged in the shared
// file, the root's result becomes NaN — a deadlock turns into a failed comparison, never a hung process.  ncclCommInitAll (all ranks in
// one process, one device each) exchanges at ncclGroupEnd with stream events and a host function on the root's stream that waits for nothing.
//
// Every call is appended to $FAKE_RCCL_DIR/fake_rccl.log: "<name> pid=.. rank=.. count=.. dtype=.. root=.. group=..".
// FAKE_RCCL_FAIL (read at every call): "reduce:K" — the K-th ncclReduce of the process returns 3 without exchanging anything;
// "initrank" — ncclCommInitRank returns 3.  -DFAKE_RCCL_OMIT_GROUP_END builds a variant without ncclGroupEnd.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <limits>
#include <fcntl.h>
#include <mutex>
#include <string>
#include <sys/mman.h>
#include <unistd.h>
#include <vector>

#define EXPORT extern "C" __attribute__((visibility("default")))

namespace {
enum { OK = 0, UNHANDLED_CUDA = 1, SYSTEM = 2, INTERNAL = 3, INVALID_ARG = 4 };
enum { MAX_RANKS = 8 };
const char MAGIC[8] = {'F', 'A', 'K', 'E', 'R', 'C', 'C', 'L'};

struct UniqueId {
    char internal[128];   // MAGIC | nonce (8 bytes) | NUL-terminated name of the shared file in $FAKE_RCCL_DIR
};

struct Slot {   // one per rank: its contribution to the current reduce
    std::atomic<uint64_t> posted;   // generation whose data is in this slot
    std::atomic<uint64_t> taken;    // generation the root has consumed
    uint64_t count;
    int32_t dtype, root;
};
struct Header {
    char magic[8];
    uint64_t nonce;
    uint64_t slot_bytes;
    std::atomic<int32_t> world;
    std::atomic<int32_t> arrived;   // bit per rank (ncclCommInitRank)
    std::atomic<int32_t> error;     // set by any rank whose wait timed out or whose peers disagree
    Slot slots[MAX_RANKS];
};
static_assert(sizeof(Header) <= 4096, "header fits in the first page");
const size_t DATA_OFFSET = 4096;

struct Comm {
    Header* h = nullptr;
    size_t map_bytes = 0;
    std::string path;
    int rank = 0, world = 1;
    uint64_t gen = 0;
    void* send = nullptr;   // pinned: this rank's contribution
    void* result = nullptr; // pinned: the root's sum
    size_t cap = 0;
    // ncclCommInitAll: every rank lives in this process, one device each.  Their reduces are exchanged with stream events instead of
    // waits in host functions (the runtime may run the host functions of all streams on one thread)
    bool local = false;
    int device = 0;
    hipEvent_t ev = nullptr;
};
struct Deferred {   // a reduce of a local comm inside ncclGroupStart / ncclGroupEnd
    Comm* c;
    const void* send;
    void* recv;
    size_t count;
    int dtype, root;
    hipStream_t stream;
};
struct Op {   // one enqueued exchange (the host function's argument)
    Comm* c;
    uint64_t gen;
    size_t count;
    int dtype, root;
};

int g_group_depth = 0;
long g_reduce_calls = 0;
std::vector<Deferred> g_deferred;
std::mutex g_mu;

std::string dir() {
    const char* d = std::getenv("FAKE_RCCL_DIR");
    return d && *d ? d : "/tmp";
}
double timeout_s() {
    const char* t = std::getenv("FAKE_RCCL_TIMEOUT_S");
    return t && std::atof(t) > 0 ? std::atof(t) : 60.0;
}
void log_line(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void log_line(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    int n = std::vsnprintf(buf, sizeof(buf) - 1, fmt, ap);
    va_end(ap);
    if (n < 0) return;
    if (n > (int)sizeof(buf) - 2) n = (int)sizeof(buf) - 2;
    buf[n++] = '\n';
    const int fd = ::open((dir() + "/fake_rccl.log").c_str(), O_WRONLY | O_CREAT | O_APPEND | O_CLOEXEC, 0644);
    if (fd < 0) return;
    ssize_t w = ::write(fd, buf, (size_t)n);   // one write per line: O_APPEND keeps lines of concurrent ranks whole
    (void)w;
    ::close(fd);
}
bool injected(const char* what, long k) {
    const char* f = std::getenv("FAKE_RCCL_FAIL");
    if (!f) return false;
    const size_t n = std::strlen(what);
    if (std::strncmp(f, what, n) != 0) return false;
    if (f[n] == '\0') return k < 0;
    return f[n] == ':' && k >= 0 && std::atol(f + n + 1) == k;
}
double now() {
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec + 1e-9 * t.tv_nsec;
}
template <class Pred>
bool wait_until(Pred pred) {
    const double end = now() + timeout_s();
    const timespec nap = {0, 50000};
    while (!pred()) {
        if (now() > end) return false;
        nanosleep(&nap, nullptr);
    }
    return true;
}
size_t elt_bytes(int dtype) { return dtype == 8 ? 8 : 4; }
char* slot_data(Comm* c, int r) { return reinterpret_cast<char*>(c->h) + DATA_OFFSET + (size_t)r * c->h->slot_bytes; }

int map_shared(const std::string& path, Comm* c) {
    const int fd = ::open(path.c_str(), O_RDWR | O_CLOEXEC);
    if (fd < 0) return SYSTEM;
    const off_t size = ::lseek(fd, 0, SEEK_END);
    void* p = size > 0 ? ::mmap(nullptr, (size_t)size, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0) : MAP_FAILED;
    ::close(fd);
    if (p == MAP_FAILED) return SYSTEM;
    c->h = static_cast<Header*>(p);
    c->map_bytes = (size_t)size;
    c->path = path;
    return OK;
}
int make_id(UniqueId* id) {
    uint64_t nonce = ((uint64_t)getpid() << 32) ^ (uint64_t)(now() * 1e9);
    char name[64];
    const int n = std::snprintf(name, sizeof(name), "fake_rccl_%016llx.shm", (unsigned long long)nonce);
    if (n < 0 || n >= (int)sizeof(name)) return INTERNAL;
    const std::string path = dir() + "/" + name;
    const char* sb = std::getenv("FAKE_RCCL_SLOT_BYTES");
    const uint64_t slot_bytes = sb && std::atoll(sb) > 0 ? (uint64_t)std::atoll(sb) : (4u << 20);
    const int fd = ::open(path.c_str(), O_RDWR | O_CREAT | O_EXCL | O_CLOEXEC, 0600);
    if (fd < 0) return SYSTEM;
    if (::ftruncate(fd, (off_t)(DATA_OFFSET + MAX_RANKS * slot_bytes)) != 0) {   // (sparse: only the slots used take memory)
        ::close(fd);
        return SYSTEM;
    }
    Header h0;
    std::memset(static_cast<void*>(&h0), 0, sizeof(h0));
    std::memcpy(h0.magic, MAGIC, 8);
    h0.nonce = nonce;
    h0.slot_bytes = slot_bytes;
    const bool ok = ::pwrite(fd, &h0, sizeof(h0), 0) == (ssize_t)sizeof(h0);
    ::close(fd);
    if (!ok) return SYSTEM;
    std::memset(id->internal, 0, sizeof(id->internal));
    std::memcpy(id->internal, MAGIC, 8);
    std::memcpy(id->internal + 8, &nonce, 8);
    std::memcpy(id->internal + 16, name, (size_t)n + 1);
    return OK;
}
int attach(Comm* c, const UniqueId& id, int world, int rank) {
    if (std::memcmp(id.internal, MAGIC, 8) != 0 || world < 1 || world > MAX_RANKS || rank < 0 || rank >= world) return INVALID_ARG;
    char name[113];
    std::memcpy(name, id.internal + 16, 112);
    name[112] = '\0';
    if (!name[0] || std::strchr(name, '/')) return INVALID_ARG;
    if (int e = map_shared(dir() + "/" + name, c)) return e;
    uint64_t nonce;
    std::memcpy(&nonce, id.internal + 8, 8);
    if (std::memcmp(c->h->magic, MAGIC, 8) != 0 || c->h->nonce != nonce) return INVALID_ARG;
    int expect = 0;
    if (!c->h->world.compare_exchange_strong(expect, world) && expect != world) return INVALID_ARG;
    c->rank = rank;
    c->world = world;
    c->h->arrived.fetch_or(1 << rank);
    return OK;
}
void detach(Comm* c) {
    if (c->h) ::munmap(c->h, c->map_bytes);
    if (c->send) (void)hipHostFree(c->send);
    if (c->result) (void)hipHostFree(c->result);
    if (c->ev) (void)hipEventDestroy(c->ev);
    delete c;
}

template <class T>
void sum_ranks(void* result, const std::vector<const void*>& src, size_t count) {
    T* out = static_cast<T*>(result);
    std::memcpy(out, src[0], count * sizeof(T));
    for (size_t r = 1; r < src.size(); ++r) {   // rank order 0, 1, ..., world-1, in the element type
        const T* in = static_cast<const T*>(src[r]);
        for (size_t i = 0; i < count; ++i) out[i] = out[i] + in[i];
    }
}
void sum_any(int dtype, void* result, const std::vector<const void*>& src, size_t count) {
    if (dtype == 8) sum_ranks<double>(result, src, count);
    else sum_ranks<float>(result, src, count);
}
template <class T>
void fill_nan(void* p, size_t count) {
    T* out = static_cast<T*>(p);
    for (size_t i = 0; i < count; ++i) out[i] = std::numeric_limits<T>::quiet_NaN();
}
void fail_op(Comm* c, const Op& op, const char* why) {
    c->h->error.store(1);
    log_line("ERROR %s pid=%d rank=%d gen=%llu", why, (int)getpid(), c->rank, (unsigned long long)op.gen);
    if (c->rank == op.root) {
        if (op.dtype == 8) fill_nan<double>(c->result, op.count);
        else fill_nan<float>(c->result, op.count);
    }
}

// the host function of one ncclReduce: runs in stream order after the device -> pinned copy; no HIP calls
void exchange(void* arg) {
    Op op = *static_cast<Op*>(arg);
    delete static_cast<Op*>(arg);
    Comm* c = op.c;
    Slot& mine = c->h->slots[c->rank];
    std::memcpy(slot_data(c, c->rank), c->send, op.count * elt_bytes(op.dtype));
    mine.count = op.count;
    mine.dtype = op.dtype;
    mine.root = op.root;
    mine.posted.store(op.gen, std::memory_order_release);
    if (c->rank == op.root) {
        for (int r = 0; r < c->world; ++r)
            if (!wait_until([&] { return c->h->slots[r].posted.load(std::memory_order_acquire) >= op.gen; })) return fail_op(c, op, "timeout waiting for a rank's data");
        for (int r = 0; r < c->world; ++r) {
            const Slot& s = c->h->slots[r];
            if (s.posted.load() != op.gen || s.count != op.count || s.dtype != op.dtype || s.root != op.root) {
                for (int q = 0; q < c->world; ++q) c->h->slots[q].taken.store(op.gen, std::memory_order_release);
                return fail_op(c, op, "ranks disagree on generation, count, dtype or root");
            }
        }
        std::vector<const void*> src;
        for (int r = 0; r < c->world; ++r) src.push_back(slot_data(c, r));
        sum_any(op.dtype, c->result, src, op.count);
        for (int r = 0; r < c->world; ++r) c->h->slots[r].taken.store(op.gen, std::memory_order_release);
    } else if (!wait_until([&] { return mine.taken.load(std::memory_order_acquire) >= op.gen; })) {
        fail_op(c, op, "timeout waiting for the root");
    }
}
int grow(Comm* c, size_t bytes, hipStream_t stream) {
    if (bytes <= c->cap) return OK;
    // earlier exchanges of this comm may still read the buffers: the stream drains first
    if (hipStreamSynchronize(stream) != hipSuccess) return UNHANDLED_CUDA;
    if (c->send) (void)hipHostFree(c->send);
    if (c->result) (void)hipHostFree(c->result);
    c->send = c->result = nullptr;
    c->cap = 0;
    if (hipHostMalloc(&c->send, bytes, hipHostMallocDefault) != hipSuccess || hipHostMalloc(&c->result, bytes, hipHostMallocDefault) != hipSuccess)
        return UNHANDLED_CUDA;
    c->cap = bytes;
    return OK;
}

struct LocalSum {   // the root's host function of a local exchange: every rank's copy is complete (stream events), nothing to wait for
    std::vector<const void*> src;
    void* result;
    size_t count;
    int dtype;
};
void local_sum(void* arg) {
    LocalSum* s = static_cast<LocalSum*>(arg);
    sum_any(s->dtype, s->result, s->src, s->count);
    delete s;
}
// all ranks of a local comm: device -> pinned on every stream, the root's stream waits for them, sums, copies to recvbuff; every other
// stream then waits for the root (its send buffer is free again)
int run_local(std::vector<Deferred>& ops) {
    const int world = ops.empty() ? 0 : ops[0].c->world;
    if ((int)ops.size() != world) return INVALID_ARG;
    std::vector<Deferred*> by_rank(world, nullptr);
    for (Deferred& d : ops) {
        if (d.c->h != ops[0].c->h || by_rank[d.c->rank] || d.count != ops[0].count || d.dtype != ops[0].dtype || d.root != ops[0].root)
            return INVALID_ARG;
        by_rank[d.c->rank] = &d;
    }
    const size_t bytes = ops[0].count * elt_bytes(ops[0].dtype);
    for (Deferred* d : by_rank) {
        if (hipSetDevice(d->c->device) != hipSuccess) return UNHANDLED_CUDA;
        if (int e = grow(d->c, bytes, d->stream)) return e;
        if (hipMemcpyAsync(d->c->send, d->send, bytes, hipMemcpyDeviceToHost, d->stream) != hipSuccess) return UNHANDLED_CUDA;
        if (hipEventRecord(d->c->ev, d->stream) != hipSuccess) return UNHANDLED_CUDA;
    }
    Deferred* root = by_rank[ops[0].root];
    if (hipSetDevice(root->c->device) != hipSuccess) return UNHANDLED_CUDA;
    LocalSum* s = new LocalSum{{}, root->c->result, root->count, root->dtype};
    for (Deferred* d : by_rank) {
        s->src.push_back(d->c->send);
        if (d != root && hipStreamWaitEvent(root->stream, d->c->ev, 0) != hipSuccess) {
            delete s;
            return UNHANDLED_CUDA;
        }
    }
    if (hipLaunchHostFunc(root->stream, local_sum, s) != hipSuccess) {
        delete s;
        return UNHANDLED_CUDA;
    }
    if (hipMemcpyAsync(root->recv, root->c->result, bytes, hipMemcpyHostToDevice, root->stream) != hipSuccess) return UNHANDLED_CUDA;
    if (hipEventRecord(root->c->ev, root->stream) != hipSuccess) return UNHANDLED_CUDA;
    for (Deferred* d : by_rank) {
        if (d == root) continue;
        if (hipSetDevice(d->c->device) != hipSuccess || hipStreamWaitEvent(d->stream, root->c->ev, 0) != hipSuccess) return UNHANDLED_CUDA;
    }
    return OK;
}
}  // namespace

EXPORT const char* ncclGetErrorString(int code) {
    switch (code) {
        case OK: return "fake rccl: no error";
        case UNHANDLED_CUDA: return "fake rccl: HIP call failed";
        case SYSTEM: return "fake rccl: system error (shared file)";
        case INTERNAL: return "fake rccl: injected failure";
        case INVALID_ARG: return "fake rccl: invalid argument";
        default: return "fake rccl: unknown error";
    }
}

EXPORT int ncclGetUniqueId(UniqueId* id) {
    if (!id) return INVALID_ARG;
    const int e = make_id(id);
    log_line("ncclGetUniqueId pid=%d rank=-1 count=0 dtype=0 root=0 group=%d rc=%d", (int)getpid(), g_group_depth, e);
    return e;
}

EXPORT int ncclCommInitRank(void** comm, int world, UniqueId id, int rank) {
    log_line("ncclCommInitRank pid=%d rank=%d count=0 dtype=0 root=0 group=%d world=%d", (int)getpid(), rank, g_group_depth, world);
    if (!comm) return INVALID_ARG;
    if (injected("initrank", -1)) return INTERNAL;
    Comm* c = new Comm();
    if (int e = attach(c, id, world, rank)) {
        detach(c);
        return e;
    }
    const int all = (1 << world) - 1;
    if (!wait_until([&] { return c->h->arrived.load() == all; })) {
        c->h->error.store(1);
        log_line("ERROR timeout in ncclCommInitRank pid=%d rank=%d", (int)getpid(), rank);
        detach(c);
        return SYSTEM;
    }
    *comm = c;
    return OK;
}

// all ranks in this process (the one-process-many-GPUs layout): one shared file, every rank arrives at once
EXPORT int ncclCommInitAll(void** comms, int n, const int* devlist) {
    log_line("ncclCommInitAll pid=%d rank=-1 count=0 dtype=0 root=0 group=%d world=%d", (int)getpid(), g_group_depth, n);
    if (!comms || n < 1 || n > MAX_RANKS) return INVALID_ARG;
    UniqueId id;
    if (int e = make_id(&id)) return e;
    for (int r = 0; r < n; ++r) {
        Comm* c = new Comm();
        if (int e = attach(c, id, n, r)) {
            detach(c);
            for (int q = 0; q < r; ++q) detach(static_cast<Comm*>(comms[q]));
            return e;
        }
        c->local = true;
        c->device = devlist ? devlist[r] : r;
        if (hipSetDevice(c->device) != hipSuccess || hipEventCreateWithFlags(&c->ev, hipEventDisableTiming) != hipSuccess) {
            detach(c);
            for (int q = 0; q < r; ++q) detach(static_cast<Comm*>(comms[q]));
            return UNHANDLED_CUDA;
        }
        comms[r] = c;
    }
    return OK;
}

EXPORT int ncclCommDestroy(void* comm) {
    Comm* c = static_cast<Comm*>(comm);
    log_line("ncclCommDestroy pid=%d rank=%d count=0 dtype=0 root=0 group=%d", (int)getpid(), c ? c->rank : -1, g_group_depth);
    if (!c) return INVALID_ARG;
    detach(c);
    return OK;
}

EXPORT int ncclReduce(const void* sendbuff, void* recvbuff, size_t count, int dtype, int op, int root, void* comm, hipStream_t stream) {
    Comm* c = static_cast<Comm*>(comm);
    long k;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        k = ++g_reduce_calls;
    }
    log_line("ncclReduce pid=%d rank=%d count=%zu dtype=%d root=%d group=%d op=%d", (int)getpid(), c ? c->rank : -1, count, dtype, root,
             g_group_depth, op);
    if (injected("reduce", k)) return INTERNAL;
    if (!c || !sendbuff || (dtype != 7 && dtype != 8) || op != 0 || root < 0 || root >= c->world) return INVALID_ARG;
    if (c->rank == root && !recvbuff) return INVALID_ARG;
    const size_t bytes = count * elt_bytes(dtype);
    if (bytes > c->h->slot_bytes) return INVALID_ARG;
    if (c->local) {
        g_deferred.push_back(Deferred{c, sendbuff, recvbuff, count, dtype, root, stream});
        if (g_group_depth > 0) return OK;   // exchanged by the outermost ncclGroupEnd
        const int e = run_local(g_deferred);
        g_deferred.clear();
        return e;
    }
    if (int e = grow(c, bytes, stream)) return e;
    if (hipMemcpyAsync(c->send, sendbuff, bytes, hipMemcpyDeviceToHost, stream) != hipSuccess) return UNHANDLED_CUDA;
    Op* o = new Op{c, ++c->gen, count, dtype, root};
    if (hipLaunchHostFunc(stream, exchange, o) != hipSuccess) {
        delete o;
        return UNHANDLED_CUDA;
    }
    if (c->rank == root && hipMemcpyAsync(recvbuff, c->result, bytes, hipMemcpyHostToDevice, stream) != hipSuccess) return UNHANDLED_CUDA;
    return OK;
}

EXPORT int ncclGroupStart() {
    ++g_group_depth;
    log_line("ncclGroupStart pid=%d rank=-1 count=0 dtype=0 root=0 group=%d", (int)getpid(), g_group_depth);
    return OK;
}

#ifndef FAKE_RCCL_OMIT_GROUP_END
EXPORT int ncclGroupEnd() {
    log_line("ncclGroupEnd pid=%d rank=-1 count=0 dtype=0 root=0 group=%d", (int)getpid(), g_group_depth);
    if (g_group_depth < 1) return INVALID_ARG;
    if (--g_group_depth > 0 || g_deferred.empty()) return OK;
    const int e = run_local(g_deferred);
    g_deferred.clear();
    return e;
}
#endif
