// stub_hip_vp.cpp -- the two runtime functions that cpp/VideoProcessor.cpp calls beyond the library's 23 (stub_hip.cpp): kept apart so that the list the
// library links against stays exactly the library's.  Linked into hc_threads only.
#include <hip/hip_runtime_api.h>

extern "C" {
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t event, unsigned) { return event ? hipSuccess : hipErrorInvalidHandle; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
}
