// The launch check of the libraries that report "<entry point>: launch failed: <HIP's text>".  HIP, so for .hip files only.
#pragma once
#include <hip/hip_runtime.h>

// Once per library, inside its namespace, where its set_error (HOST_ARGS_DEFINE_ERROR_TEXT) is declared: an entry point
// ends with `return launched("its name")` behind its last launch.  1 after a failed launch, with the text set; else 0.
#define LAUNCH_CHECK_DEFINE_LAUNCHED()                                   \
  int launched(const char* what) {                                      \
    const hipError_t e = hipGetLastError();                             \
    if (e != hipSuccess) {                                              \
      set_error("%s: launch failed: %s", what, hipGetErrorString(e));   \
      return 1;                                                         \
    }                                                                   \
    return 0;                                                           \
  }
