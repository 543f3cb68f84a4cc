// hc_stub.h -- what the host-check drivers (hc_*.cpp) ask of stub_hip.cpp beyond the HIP runtime's own functions.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

// One launch as the stub saw it (hipLaunchKernel / hipExtLaunchKernel); nothing is ever executed.
struct HcLaunch {
    const void *fn;   // host function, as registered by the translation unit that defines the kernel
    const char *name; // its device name (mangled), "" for a function nobody registered
    unsigned grid[3], block[3];
    size_t lds;       // dynamic LDS bytes
    hipStream_t stream;
    int any_order;    // hipExtAnyOrderLaunch
    int captured;     // the stream was capturing
    int refused;      // the stub answered hipErrorInvalidConfiguration / hipErrorInvalidDeviceFunction
};

extern "C" {
// the "capturing" flag of a stream (nullptr: the null stream)
void hc_stub_set_capturing(hipStream_t stream, int on);
// the n-th call from now (1 = the next) of hipMalloc / hipHostMalloc / hipStreamCreate / hipEventCreateWithFlags answers hipErrorOutOfMemory; 0 = never
void hc_stub_fail_alloc_after(long n);
// the next hipEventSynchronize fails, and its event stays unwaitable from then on -- as an event recorded into a capture is
void hc_stub_poison_next_wait(void);
// the calling thread's launch log
size_t hc_stub_launch_count(void);
const HcLaunch *hc_stub_launch(size_t i);
void hc_stub_clear_launches(void);
// launches of all threads since the process began
long hc_stub_total_launches(void);
// what the stub refused or found wrong, all threads: launch configurations out of range, launches of unregistered functions, hipFree / hipMemcpy / hipMemset of
// an address it never handed out, events and streams it does not know
long hc_stub_violations(void);
// blocks, streams and events handed out and not yet returned
long hc_stub_live(void);
// prints both counts (and what is still live) on stderr; returns violations + live: a driver's last word
long hc_stub_report(const char *who);
}
