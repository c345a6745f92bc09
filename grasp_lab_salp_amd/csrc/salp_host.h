// salp_host.h — host-side error plumbing of the units that define the C ABI
// of include/salp.h: an entry point validates, launches and reports through
// these, whichever unit it lives in.  Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/salp.h"

// Hidden: none of this is exported from the library.
namespace salp __attribute__((visibility("hidden"))) {

// The text behind salp_last_error(NULL), one per thread; defined in salp_kernels.hip.
extern thread_local std::string g_last_error;

inline int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

inline int check_hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return SALP_OK;
    return fail(SALP_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace salp
