// stub_hip.cpp -- a CPU stand-in for the HIP runtime, for the host checks (tests/hostcheck/): the 23 runtime functions and the 5 registration hooks that
// libtsvpp's host side needs, and nothing else -- a new HIP call in the library fails the link of the drivers and gets noticed
// (tests/test_hostcheck_cpu.py also compares the lists).
//   memory    "device" and pinned allocations are ordinary heap blocks: AddressSanitizer sees every host write into them, every over-long copy, every double
//             free.  A registry of live blocks: hipFree / hipMemcpy / hipMemset of an address the stub never handed out is a violation.
//   launches  recorded per thread, never executed; refused (hipErrorInvalidConfiguration) outside what the real runtime accepts.
//   streams   carry a "capturing" flag the driver sets; while one is set the synchronous calls answer as the real runtime does during a capture.
//   failures  a countdown makes the n-th allocation-like call answer hipErrorOutOfMemory.
#include "hc_stub.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

namespace {

constexpr size_t kLdsBytes = 160 * 1024; // what hipGetDeviceProperties reports (gfx950) and the launch check enforces
constexpr int kDevices = 2;              // two, so that a context on device 1 makes DeviceGuard switch and restore

struct Stream {
    std::atomic<int> capturing{ 0 };
};
struct Event {
    std::atomic<int> captured{ 0 };
};

// Everything global lives in one object that is created on first use and never destroyed: the registration hooks run from static constructors of the
// library's translation units, before and after any static of this file.
struct State {
    std::mutex mu;
    std::map<uintptr_t, size_t> blocks; // live "device" and pinned blocks: base -> bytes
    std::set<Stream *> streams;
    std::set<Event *> events;
    std::map<const void *, std::string> functions; // host function -> device name
    Stream null_stream;
    std::atomic<long> capturing{ 0 }; // streams whose flag is set
    std::atomic<long> violations{ 0 }, launches{ 0 };
    std::atomic<long> fail_after{ 0 };
    std::atomic<int> poison_wait{ 0 };
};
State &st() {
    static State *s = new State();
    return *s;
}

thread_local int t_device = 0;
thread_local hipError_t t_last = hipSuccess;
thread_local std::vector<HcLaunch> t_log;
struct CallConfig {
    dim3 grid, block;
    size_t lds;
    hipStream_t stream;
};
thread_local std::vector<CallConfig> t_config;

hipError_t fail(hipError_t e) {
    t_last = e;
    return e;
}
hipError_t violation(hipError_t e, const char *what, const void *p) {
    st().violations.fetch_add(1);
    std::fprintf(stderr, "stub_hip: VIOLATION %s (%p)\n", what, p);
    return fail(e);
}

Stream *stream_of(hipStream_t s) { return s ? reinterpret_cast<Stream *>(s) : &st().null_stream; }
bool known_stream(hipStream_t s) {
    if (!s) return true;
    std::lock_guard<std::mutex> lk(st().mu);
    return st().streams.count(reinterpret_cast<Stream *>(s)) != 0;
}
bool known_event(hipEvent_t e) {
    std::lock_guard<std::mutex> lk(st().mu);
    return st().events.count(reinterpret_cast<Event *>(e)) != 0;
}
bool capturing_anywhere() { return st().capturing.load() > 0; }

// the injected failure: true when THIS call is the one to fail
bool injected() {
    long n = st().fail_after.load();
    while (n > 0) {
        if (st().fail_after.compare_exchange_weak(n, n - 1)) return n == 1;
    }
    return false;
}

// [p, p + n) lies inside one live block
bool inside_block(const void *p, size_t n) {
    const uintptr_t a = (uintptr_t)p;
    std::lock_guard<std::mutex> lk(st().mu);
    auto it = st().blocks.upper_bound(a);
    if (it == st().blocks.begin()) return false;
    --it;
    return a >= it->first && a - it->first <= it->second && n <= it->second - (a - it->first);
}

hipError_t alloc_block(void **ptr, size_t bytes) {
    if (!ptr) return fail(hipErrorInvalidValue);
    *ptr = nullptr;
    if (injected()) return fail(hipErrorOutOfMemory);
    if (bytes == 0) return hipSuccess;
    // 256-byte aligned, as the real allocator's blocks are (the library's alignment classes are decided on the addresses); the size is NOT rounded up, so the
    // sanitizer's red zone begins at the first byte past what was asked for
    void *p = nullptr;
    if (posix_memalign(&p, 256, bytes) != 0) return fail(hipErrorOutOfMemory);
    std::memset(p, 0xA5, bytes);
    std::lock_guard<std::mutex> lk(st().mu);
    st().blocks[(uintptr_t)p] = bytes;
    *ptr = p;
    return hipSuccess;
}
hipError_t free_block(void *p, const char *what) {
    if (!p) return hipSuccess;
    {
        std::lock_guard<std::mutex> lk(st().mu);
        auto it = st().blocks.find((uintptr_t)p);
        if (it != st().blocks.end()) {
            st().blocks.erase(it);
            std::free(p);
            return hipSuccess;
        }
    }
    return violation(hipErrorInvalidValue, what, p);
}

hipError_t copy(void *dst, const void *src, size_t n, hipMemcpyKind kind, const char *what) {
    if (n == 0) return hipSuccess;
    if (!dst || !src) return fail(hipErrorInvalidValue);
    const bool d = inside_block(dst, 1), s = inside_block(src, 1); // (the extent is AddressSanitizer's to judge: memcpy below)
    bool ok = true;
    switch (kind) {
    case hipMemcpyHostToDevice: ok = d; break;
    case hipMemcpyDeviceToHost: ok = s; break;
    case hipMemcpyDeviceToDevice: ok = d && s; break;
    case hipMemcpyHostToHost: break;
    default: ok = d || s; break;
    }
    if (!ok) return violation(hipErrorInvalidValue, what, d ? src : dst);
    std::memcpy(dst, src, n);
    return hipSuccess;
}

hipError_t launch(const void *fn, dim3 grid, dim3 block, size_t lds, hipStream_t stream, int any_order) {
    HcLaunch l = {};
    l.fn = fn;
    l.name = "";
    l.grid[0] = grid.x, l.grid[1] = grid.y, l.grid[2] = grid.z;
    l.block[0] = block.x, l.block[1] = block.y, l.block[2] = block.z;
    l.lds = lds;
    l.stream = stream;
    l.any_order = any_order;
    hipError_t e = hipSuccess;
    if (!known_stream(stream)) e = violation(hipErrorInvalidHandle, "launch on a stream the stub does not know", stream);
    l.captured = (e == hipSuccess && stream_of(stream)->capturing.load()) ? 1 : 0;
    {
        std::lock_guard<std::mutex> lk(st().mu);
        auto it = st().functions.find(fn);
        if (it != st().functions.end()) l.name = it->second.c_str(); // (entries are never erased: the pointer stays good)
    }
    if (!l.name[0]) e = violation(hipErrorInvalidDeviceFunction, "launch of a function no translation unit registered", fn);
    const unsigned long long threads = (unsigned long long)block.x * block.y * block.z;
    const unsigned long long groups = (unsigned long long)grid.x * grid.y * grid.z;
    if (threads < 1 || threads > 1024) e = violation(hipErrorInvalidConfiguration, "block size outside 1..1024", fn);
    else if (grid.x == 0 || grid.y == 0 || grid.z == 0) e = violation(hipErrorInvalidConfiguration, "a grid dimension of zero", fn);
    else if (groups * threads >= (1ull << 31)) e = violation(hipErrorInvalidConfiguration, "grid x block of 2^31 threads or more", fn);
    else if (lds > kLdsBytes) e = violation(hipErrorInvalidConfiguration, "dynamic LDS above 160 KiB", fn);
    l.refused = e != hipSuccess;
    t_log.push_back(l);
    st().launches.fetch_add(1);
    return e;
}

} // namespace

// ---- the drivers' side ---------------------------------------------------------------------------------------------------------------------------------------
extern "C" {

void hc_stub_set_capturing(hipStream_t stream, int on) {
    const int was = stream_of(stream)->capturing.exchange(on ? 1 : 0);
    st().capturing.fetch_add((on ? 1 : 0) - was);
}
void hc_stub_fail_alloc_after(long n) { st().fail_after.store(n); }
void hc_stub_poison_next_wait(void) { st().poison_wait.store(1); }
size_t hc_stub_launch_count(void) { return t_log.size(); }
const HcLaunch *hc_stub_launch(size_t i) { return i < t_log.size() ? &t_log[i] : nullptr; }
void hc_stub_clear_launches(void) { t_log.clear(); }
long hc_stub_total_launches(void) { return st().launches.load(); }
long hc_stub_violations(void) { return st().violations.load(); }
long hc_stub_live(void) {
    std::lock_guard<std::mutex> lk(st().mu);
    return (long)(st().blocks.size() + st().streams.size() + st().events.size());
}
long hc_stub_report(const char *who) {
    long blocks, streams, events;
    {
        std::lock_guard<std::mutex> lk(st().mu);
        blocks = (long)st().blocks.size(), streams = (long)st().streams.size(), events = (long)st().events.size();
    }
    const long v = hc_stub_violations();
    std::fprintf(stderr, "stub_hip: %s: %ld launches, %ld violations, still live: %ld blocks %ld streams %ld events\n", who, hc_stub_total_launches(), v, blocks,
                 streams, events);
    return v + blocks + streams + events;
}

// ---- registration hooks (what clang emits into every translation unit that holds a kernel) -------------------------------------------------------------------
void **__hipRegisterFatBinary(const void *) {
    static void *handle = nullptr;
    (void)st();
    return &handle;
}
void __hipRegisterFunction(void **, const void *host_function, char *, const char *device_name, unsigned, void *, void *, void *, void *, int *) {
    std::lock_guard<std::mutex> lk(st().mu);
    st().functions[host_function] = device_name ? device_name : "(unnamed)";
}
void __hipUnregisterFatBinary(void **) {}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t stream) {
    t_config.push_back(CallConfig{ grid, block, lds, stream });
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *lds, hipStream_t *stream) {
    if (t_config.empty()) return violation(hipErrorInvalidValue, "call configuration popped that nobody pushed", nullptr);
    const CallConfig c = t_config.back();
    t_config.pop_back();
    *grid = c.grid;
    *block = c.block;
    *lds = c.lds;
    *stream = c.stream;
    return hipSuccess;
}

// ---- the 23 runtime functions --------------------------------------------------------------------------------------------------------------------------------
hipError_t hipLaunchKernel(const void *fn, dim3 grid, dim3 block, void **, size_t lds, hipStream_t stream) { return launch(fn, grid, block, lds, stream, 0); }
hipError_t hipExtLaunchKernel(const void *fn, dim3 grid, dim3 block, void **, size_t lds, hipStream_t stream, hipEvent_t, hipEvent_t, int flags) {
    return launch(fn, grid, block, lds, stream, (flags & hipExtAnyOrderLaunch) ? 1 : 0);
}
hipError_t hipGetLastError(void) {
    const hipError_t e = t_last;
    t_last = hipSuccess;
    return e;
}
const char *hipGetErrorString(hipError_t e) {
    switch (e) {
    case hipSuccess: return "no error";
    case hipErrorOutOfMemory: return "out of memory";
    case hipErrorInvalidValue: return "invalid argument";
    case hipErrorInvalidDevice: return "invalid device ordinal";
    case hipErrorInvalidConfiguration: return "invalid configuration argument";
    case hipErrorInvalidDeviceFunction: return "invalid device function";
    case hipErrorInvalidHandle: return "invalid resource handle";
    case hipErrorStreamCaptureUnsupported: return "operation not permitted when stream is capturing";
    case hipErrorCapturedEvent: return "operation not permitted on an event last recorded in a capturing stream";
    default: return "stub_hip: some other error";
    }
}

hipError_t hipGetDevice(int *device) {
    if (!device) return fail(hipErrorInvalidValue);
    *device = t_device;
    return hipSuccess;
}
hipError_t hipSetDevice(int device) {
    if (device < 0 || device >= kDevices) return fail(hipErrorInvalidDevice);
    t_device = device;
    return hipSuccess;
}
hipError_t hipGetDeviceCount(int *count) {
    if (!count) return fail(hipErrorInvalidValue);
    *count = kDevices;
    return hipSuccess;
}
hipError_t hipGetDeviceProperties(hipDeviceProp_t *prop, int device) { // (the header's macro gives this its versioned symbol)
    if (!prop || device < 0 || device >= kDevices) return fail(hipErrorInvalidDevice);
    std::memset(prop, 0, sizeof(*prop));
    std::snprintf(prop->name, sizeof(prop->name), "stub MI355X");
    std::snprintf(prop->gcnArchName, sizeof(prop->gcnArchName), "gfx950");
    prop->multiProcessorCount = 256;
    prop->sharedMemPerBlock = kLdsBytes;
    prop->maxSharedMemoryPerMultiProcessor = kLdsBytes;
    prop->maxThreadsPerBlock = 1024;
    prop->warpSize = 64;
    prop->totalGlobalMem = (size_t)288 << 30;
    return hipSuccess;
}

hipError_t hipStreamCreate(hipStream_t *stream) {
    if (!stream) return fail(hipErrorInvalidValue);
    *stream = nullptr;
    if (injected()) return fail(hipErrorOutOfMemory);
    Stream *s = new Stream();
    std::lock_guard<std::mutex> lk(st().mu);
    st().streams.insert(s);
    *stream = reinterpret_cast<hipStream_t>(s);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t stream) {
    Stream *s = reinterpret_cast<Stream *>(stream);
    {
        std::lock_guard<std::mutex> lk(st().mu);
        if (!stream || st().streams.erase(s) == 0) s = nullptr;
    }
    if (!s) return violation(hipErrorInvalidHandle, "hipStreamDestroy of a stream the stub does not know", stream);
    if (s->capturing.load()) st().capturing.fetch_sub(1);
    delete s;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t stream) {
    if (!known_stream(stream)) return violation(hipErrorInvalidHandle, "hipStreamSynchronize of a stream the stub does not know", stream);
    if (stream_of(stream)->capturing.load()) return fail(hipErrorStreamCaptureUnsupported);
    return hipSuccess;
}
hipError_t hipStreamIsCapturing(hipStream_t stream, hipStreamCaptureStatus *status) {
    if (!status) return fail(hipErrorInvalidValue);
    if (!known_stream(stream)) return violation(hipErrorInvalidHandle, "hipStreamIsCapturing of a stream the stub does not know", stream);
    *status = stream_of(stream)->capturing.load() ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
    return hipSuccess;
}

hipError_t hipMalloc(void **ptr, size_t bytes) {
    if (capturing_anywhere()) return fail(hipErrorStreamCaptureUnsupported);
    return alloc_block(ptr, bytes);
}
hipError_t hipFree(void *ptr) {
    if (ptr && capturing_anywhere()) return fail(hipErrorStreamCaptureUnsupported);
    return free_block(ptr, "hipFree of an address the stub never handed out (or freed already)");
}
hipError_t hipHostMalloc(void **ptr, size_t bytes, unsigned) { return alloc_block(ptr, bytes); }
hipError_t hipHostFree(void *ptr) { return free_block(ptr, "hipHostFree of an address the stub never handed out (or freed already)"); }

hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind kind) {
    if (capturing_anywhere()) return fail(hipErrorStreamCaptureUnsupported);
    return copy(dst, src, n, kind, "hipMemcpy with no block of the stub's on its device side");
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t stream) {
    if (!known_stream(stream)) return violation(hipErrorInvalidHandle, "hipMemcpyAsync on a stream the stub does not know", stream);
    return copy(dst, src, n, kind, "hipMemcpyAsync with no block of the stub's on its device side"); // (a capturing stream: the node's copy, done now)
}
hipError_t hipMemset(void *dst, int value, size_t n) {
    if (capturing_anywhere()) return fail(hipErrorStreamCaptureUnsupported);
    if (n == 0) return hipSuccess;
    if (!inside_block(dst, 1)) return violation(hipErrorInvalidValue, "hipMemset of an address the stub never handed out", dst);
    std::memset(dst, value, n);
    return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t *event, unsigned) {
    if (!event) return fail(hipErrorInvalidValue);
    *event = nullptr;
    if (injected()) return fail(hipErrorOutOfMemory);
    Event *e = new Event();
    std::lock_guard<std::mutex> lk(st().mu);
    st().events.insert(e);
    *event = reinterpret_cast<hipEvent_t>(e);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t event) {
    Event *e = reinterpret_cast<Event *>(event);
    {
        std::lock_guard<std::mutex> lk(st().mu);
        if (!event || st().events.erase(e) == 0) e = nullptr;
    }
    if (!e) return violation(hipErrorInvalidHandle, "hipEventDestroy of an event the stub does not know", event);
    delete e;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream) {
    if (!event || !known_event(event)) return violation(hipErrorInvalidHandle, "hipEventRecord of an event the stub does not know", event);
    if (!known_stream(stream)) return violation(hipErrorInvalidHandle, "hipEventRecord on a stream the stub does not know", stream);
    reinterpret_cast<Event *>(event)->captured.store(stream_of(stream)->capturing.load());
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t event) {
    if (!event || !known_event(event)) return violation(hipErrorInvalidHandle, "hipEventSynchronize of an event the stub does not know", event);
    if (st().poison_wait.exchange(0)) reinterpret_cast<Event *>(event)->captured.store(1);
    if (reinterpret_cast<Event *>(event)->captured.load()) return fail(hipErrorCapturedEvent);
    return hipSuccess;
}

} // extern "C"
