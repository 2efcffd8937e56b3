// dronerl_host.h — the host API units' way to refuse a call (the *_api.cpp units only: no .hip unit includes
// this).  The message lands in drl_last_error through dronerl_api.cpp, which keeps the printf-style original.
#ifndef DRONERL_HOST_H
#define DRONERL_HOST_H

#include <hip/hip_runtime.h>
#include <stdio.h>

extern "C" __attribute__((visibility("hidden"))) int drl_internal_fail(const char* msg);

namespace drl {

// -1, with `m` as the thread's last error
__attribute__((visibility("hidden"))) inline int fail(const char* m) { return drl_internal_fail(m); }

// ... with "<what>: <HIP's text for e>" (e: a hipError_t, or the int a launch_* function returns one as)
__attribute__((visibility("hidden"))) inline int hip_fail(int e, const char* what) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString((hipError_t)e));
    return fail(buf);
}

}  // namespace drl
#endif
