// Error reporting of libdeva_hip.so for host code: no HIP in here, so the translation units that only decide or pack
// (conv_plan.cpp, conv_pack.cpp) compile with the host compiler alone.  common.h includes it for everything else.
#pragma once
#include "host_args.h"

namespace deva {
using namespace host_args;

void set_error(const char* fmt, ...);  // runtime.hip; text behind deva_hip_last_error()

#define DEVA_REQUIRE(cond, ...) HOST_ARGS_REQUIRE(deva::set_error, cond, __VA_ARGS__)

}  // namespace deva
