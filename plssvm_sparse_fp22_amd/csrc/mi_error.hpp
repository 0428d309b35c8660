// The error carrier of the backend, free of HIP so that host-only headers (lane_plan.hpp) and their CPU checks throw it too.
#pragma once

#include <stdexcept>
#include <string>

namespace plssvm_mi {

// Error carrier turned into a PLSSVM_MI_ERR_* code at the C ABI (the reference throws
// plssvm::hip::backend_exception from PLSSVM_HIP_ERROR_CHECK, src/plssvm/backends/HIP/detail/utility.hip.cpp:19-23).
struct mi_error : std::runtime_error {
    int code;
    mi_error(int c, const std::string &msg) : std::runtime_error(msg), code(c) {}
};

}  // namespace plssvm_mi
