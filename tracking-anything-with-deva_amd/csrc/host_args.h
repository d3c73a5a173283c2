// Host-side argument helpers of every library: pointer predicates, the scratch bump layout, and the error text and
// REQUIRE macro that each library instantiates for itself.  Header-only, internal linkage, no HIP: every *_plan.cpp
// and every tests/*_sanitize_main.cpp can include it, and no library exports or shares anything from it.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

namespace host_args {
namespace {

// the address alone: null counts as aligned, so a call site that also refuses null says `p && aligned(p, n)`
inline bool aligned(const void* p, int n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

// two byte ranges share a byte (addresses as integers: nothing is dereferenced); a null or empty range shares none
inline bool overlaps(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a && b && a_bytes > 0 && b_bytes > 0 && a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

inline int64_t round256(int64_t v) { return (v + 255) / 256 * 256; }

// a scratch buffer carved front to back, every piece on a 256-byte boundary: take() gives a piece's offset, `at` the total
struct ScratchLayout {
  int64_t at = 0;
  int64_t take(int64_t bytes) {
    const int64_t off = at;
    at += round256(bytes);
    return off;
  }
};

// the caller's scratch holds what the feature's *_scratch function asks for
inline bool scratch_ok(const void* scratch, int64_t scratch_bytes, int64_t need) {
  return scratch && aligned(scratch, 16) && scratch_bytes >= need;
}

}  // namespace
}  // namespace host_args

// Once per library, inside its namespace: the text behind its *_last_error().  The storage belongs to the translation
// unit that expands this, so no two libraries share it.
#define HOST_ARGS_DEFINE_ERROR_TEXT()              \
  static thread_local char g_err[512] = "";       \
  void set_error(const char* fmt, ...) {          \
    va_list ap;                                   \
    va_start(ap, fmt);                            \
    vsnprintf(g_err, sizeof(g_err), fmt, ap);     \
    va_end(ap);                                   \
  }

// every library's DEVA_*_REQUIRE (DEVA_REQUIRE, DEVA_METRICS_REQUIRE, ...) is this with its own set_error
#define HOST_ARGS_REQUIRE(set_error, cond, ...) \
  do {                                          \
    if (!(cond)) {                              \
      set_error(__VA_ARGS__);                   \
      return 2;                                 \
    }                                           \
  } while (0)
