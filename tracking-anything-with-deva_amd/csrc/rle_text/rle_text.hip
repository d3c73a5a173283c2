// deva_text_encode_count, deva_text_encode_write and deva_text_parse (include/deva_rle_text.h, rules C1-C8): the text of
// COCO run-length masks coded from run boundaries and parsed into the run array of deva_rle.h, on the device.
//
// Every per-mask kernel gives a workgroup one mask and walks it DEVA_TEXT_SCAN_CHUNK items a step, kItems consecutive
// items a lane, with the carries of the steps before in registers (uniform over the workgroup).
//
//   encode  text_len_kernel   item = count.  A lane reads the kItems + 3 boundaries its counts need (C3: 0 before the
//                             first, H * W from the last on and for a slot outside `bounds`), forms the values (C2) and
//                             sums their widths (C1); one reduction over the workgroup at the end.
//           text_base_kernel  one workgroup: text_len -> text_base and text_total (C4).
//           text_write_kernel the walk of text_len_kernel again; an exclusive scan of the lanes' widths plus the carry
//                             places every value, whose characters leave as byte stores below `capacity`.
//   parse   values_kernel     item = character.  Counts the characters that end a value and takes the flags CHAR and
//                             OPEN, per mask, into the scratch.
//           first_kernel      one workgroup: the value counts -> first[0 .. n], info[1], info[0] = the flags so far.
//           starts_kernel     item = character.  A lane whose character ends a value reads it back to front: at most
//                             11 characters before its own and never below the text's first, wherever the step began.
//                             Then three scans with carries: the rank of the value in its mask, the two interleaved
//                             chains of C2, and the running sum of the counts, which is the start behind the value.
//
// Every load lies inside the inputs as the arguments size them (text_first is clamped into [0, L], a boundary slot into
// [0, bounds_len)); every store lies inside text_len, text_base, text_total, chars[0, capacity), the scratch,
// runs[0, words_cap) and info, at places that depend on indices alone.
#include <hip/hip_runtime.h>

#include "../block_scan.h"
#include "../launch_check.h"
#include "rle_text_plan.h"

namespace deva_text {
namespace {

static_assert(kBlock == 256 && kItems * kBlock == DEVA_TEXT_SCAN_CHUNK && DEVA_TEXT_MASK_CHUNK == kBlock, "the walks' steps");
constexpr int kWaves = kBlock / 64;
typedef unsigned long long u64;

// -> (the sum of the lanes before this one in the workgroup, the workgroup's sum); two barriers
template <typename V>
__device__ __forceinline__ void block_exclusive(V v, V (&wave_sums)[kWaves], int tid, V& before, V& all) {
  block_scan::block_exclusive<block_scan::Sum>(v, (V)0, wave_sums, tid, before, all);
}

// ------------------------------------------------------------------------------------------ encode
struct EncodeArgs {
  const int32_t* n_in;
  const int64_t* base;
  const int32_t* bounds;
  int64_t bounds_len;
  int64_t total;   // H * W
};

// C1: characters of the canonical coding of x (1 .. 13)
__device__ __forceinline__ int value_width(long long x) {
  int width = 1;
  for (;;) {
    const int c = (int)(x & 0x1f);
    x >>= 5;
    if ((c & 0x10) ? x == -1 : x == 0) return width;
    ++width;
  }
}

// C3: boundary i of a mask of nk boundaries that begin at `base`; 0 before the first, H * W from the last on
__device__ __forceinline__ long long bound_at(const EncodeArgs& a, int64_t base, int nk, int64_t i) {
  if (i < 0) return 0;
  if (i >= nk) return a.total;
  const int64_t slot = base + i;
  return slot >= 0 && slot < a.bounds_len ? (long long)a.bounds[slot] : (long long)a.total;
}

// C2: the coded values of the counts j0 .. j0 + kItems - 1 of the mask (those below `counts`; the rest are not touched)
__device__ __forceinline__ void lane_values(const EncodeArgs& a, int64_t base, int nk, int64_t j0, long long (&v)[kItems]) {
  long long b[kItems + 3];
#pragma unroll
  for (int e = 0; e < kItems + 3; ++e) b[e] = bound_at(a, base, nk, j0 - 3 + e);
#pragma unroll
  for (int e = 0; e < kItems; ++e) {
    const long long count = b[e + 3] - b[e + 2];
    v[e] = j0 + e < 3 ? count : count - (b[e + 1] - b[e]);
  }
}

__global__ __launch_bounds__(kBlock) void text_len_kernel(EncodeArgs a, int32_t* text_len) {
  __shared__ long long wave_sums[kWaves];
  const int tid = threadIdx.x, k = blockIdx.x;
  const int nk = max(a.n_in[k], 0);
  const int64_t base = a.base[k], counts = (int64_t)nk + 1;
  long long mine = 0;
  for (int64_t begin = 0; begin < counts; begin += DEVA_TEXT_SCAN_CHUNK) {
    const int64_t j0 = begin + tid * kItems;
    if (j0 >= counts) continue;                            // (no barrier in this loop)
    long long v[kItems];
    lane_values(a, base, nk, j0, v);
#pragma unroll
    for (int e = 0; e < kItems; ++e)
      if (j0 + e < counts) mine += value_width(v[e]);
  }
  long long before, all;
  block_exclusive(mine, wave_sums, tid, before, all);
  if (tid == 0) text_len[k] = (int32_t)all;
}

// one workgroup: text_base[k] = first + text_len[0] + ... + text_len[k-1], text_total = first + all of them (C4)
__global__ __launch_bounds__(kBlock) void text_base_kernel(const int32_t* text_len, int n, const int64_t* first, int64_t* text_base,
                                                           int64_t* text_total) {
  __shared__ long long wave_sums[kWaves];
  const long long all = block_scan::block_offsets(text_len, n, first ? (long long)*first : 0ll, text_base, wave_sums, threadIdx.x);
  if (threadIdx.x == 0) *text_total = all;
}

__global__ __launch_bounds__(kBlock) void text_write_kernel(EncodeArgs a, const int64_t* text_base, uint8_t* chars, int64_t capacity) {
  __shared__ long long wave_sums[kWaves];
  const int tid = threadIdx.x, k = blockIdx.x;
  const int nk = max(a.n_in[k], 0);
  const int64_t base = a.base[k], counts = (int64_t)nk + 1;
  long long running = text_base[k];
  if (running >= capacity || running < 0) return;          // (uniform over the workgroup: nothing of this mask fits)
  for (int64_t begin = 0; begin < counts; begin += DEVA_TEXT_SCAN_CHUNK) {
    const int64_t j0 = begin + tid * kItems;
    long long v[kItems];
    long long mine = 0;
    if (j0 < counts) {
      lane_values(a, base, nk, j0, v);
#pragma unroll
      for (int e = 0; e < kItems; ++e)
        if (j0 + e < counts) mine += value_width(v[e]);
    }
    long long before, all;
    block_exclusive(mine, wave_sums, tid, before, all);
    long long slot = running + before;
    if (j0 < counts) {
#pragma unroll
      for (int e = 0; e < kItems; ++e) {
        if (j0 + e >= counts) break;
        long long x = v[e];
        for (;;) {                                         // C1
          const int c = (int)(x & 0x1f);
          x >>= 5;
          const bool more = (c & 0x10) ? x != -1 : x != 0;
          if (slot < capacity) chars[slot] = (uint8_t)((c | (more ? 0x20 : 0)) + 48);
          ++slot;
          if (!more) break;
        }
      }
    }
    running += all;
    if (running >= capacity) return;                       // (uniform: the carry is the same in every lane)
  }
}

// ------------------------------------------------------------------------------------------ parse
struct ParseArgs {
  const uint8_t* chars;
  const int64_t* text_first;
  int32_t* values;   // scratch: values of every mask
  int32_t* flags;    // scratch: flags of every mask (CHAR, OPEN)
  int32_t* runs;
  int64_t* info;
  int64_t chars_len, words_cap, total;
  int n;
};

__device__ __forceinline__ int64_t clamped(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the text of mask k: [lo, hi) inside [0, L] (C5)
__device__ __forceinline__ void text_of(const ParseArgs& a, int k, int64_t& lo, int64_t& hi) {
  lo = clamped(a.text_first[k], 0, a.chars_len);
  hi = clamped(a.text_first[k + 1], lo, a.chars_len);
}

__device__ __forceinline__ bool continues(uint8_t v) { return v <= 63 && (v & 0x20); }   // (v: the character - 48, wrapped)
__device__ __forceinline__ bool ends_value(uint8_t v) { return v <= 63 && !(v & 0x20); }

__global__ __launch_bounds__(kBlock) void values_kernel(ParseArgs a) {
  __shared__ int wave_sums[kWaves];
  __shared__ int any_flags;
  const int tid = threadIdx.x, k = blockIdx.x;
  int64_t lo, hi;
  text_of(a, k, lo, hi);
  if (tid == 0) any_flags = 0;
  int found = 0, flags = 0;
  for (int64_t begin = lo; begin < hi; begin += DEVA_TEXT_SCAN_CHUNK) {
    const int64_t p0 = begin + tid * kItems;
#pragma unroll
    for (int e = 0; e < kItems; ++e) {
      if (p0 + e < hi) {
        const uint8_t v = (uint8_t)(a.chars[p0 + e] - 48);
        found += ends_value(v);
        if (v > 63) flags |= DEVA_TEXT_FLAG_CHAR;
      }
    }
  }
  if (tid == 0 && hi > lo && continues((uint8_t)(a.chars[hi - 1] - 48))) flags |= DEVA_TEXT_FLAG_OPEN;
  int before, all;
  block_exclusive(found, wave_sums, tid, before, all);     // (its first barrier orders the store of any_flags above)
  if (flags) atomicOr(&any_flags, flags);
  __syncthreads();
  if (tid == 0) {
    a.values[k] = all;
    a.flags[k] = any_flags;
  }
}

// one workgroup: first[k] = (values[0] + 1) + ... + (values[k-1] + 1); info[1] = n + 1 + first[n]; info[0] = the flags so far
__global__ __launch_bounds__(kBlock) void first_kernel(ParseArgs a) {
  __shared__ long long wave_sums[kWaves];
  __shared__ int any_flags;
  const int tid = threadIdx.x;
  if (tid == 0) any_flags = 0;
  long long running = 0;
  int flags = 0;
  for (int begin = 0; begin < a.n; begin += DEVA_TEXT_MASK_CHUNK) {
    const int i = begin + tid;
    const long long v = i < a.n ? (long long)a.values[i] + 1 : 0ll;
    if (i < a.n) flags |= a.flags[i];
    long long before, all;
    block_exclusive(v, wave_sums, tid, before, all);
    if (i < a.n && i < a.words_cap) a.runs[i] = (int32_t)(running + before);
    running += all;
  }
  __syncthreads();                                         // (any_flags is zero before the first atomic: n may be 0)
  if (flags) atomicOr(&any_flags, flags);
  __syncthreads();
  if (tid == 0) {
    if (a.n < a.words_cap) a.runs[a.n] = (int32_t)running;
    a.info[0] = any_flags;
    a.info[1] = (long long)a.n + 1 + running;
  }
}

__global__ __launch_bounds__(kBlock) void starts_kernel(ParseArgs a) {
  __shared__ int rank_sums[kWaves];
  __shared__ u64 even_sums[kWaves], odd_sums[kWaves], start_sums[kWaves];
  const int tid = threadIdx.x, k = blockIdx.x;
  int64_t lo, hi;
  text_of(a, k, lo, hi);
  const int64_t out0 = (int64_t)a.n + 1 + a.runs[k];        // where s_0 of this mask goes (first_kernel wrote first[k])
  if (tid == 0 && out0 >= 0 && out0 < a.words_cap) a.runs[out0] = 0;
  int values = 0, flags = 0;                                // values of the mask before this step
  u64 carry_even = 0, carry_odd = 0, carry_start = 0;
  for (int64_t begin = lo; begin < hi; begin += DEVA_TEXT_SCAN_CHUNK) {
    const int64_t p0 = begin + tid * kItems;
    u64 x[kItems];
    bool is_value[kItems];
    int mine = 0;
#pragma unroll
    for (int e = 0; e < kItems; ++e) {
      const int64_t p = p0 + e;
      x[e] = 0;
      is_value[e] = false;
      if (p >= hi) continue;
      const uint8_t v = (uint8_t)(a.chars[p] - 48);
      if (!ends_value(v)) continue;
      is_value[e] = true;
      ++mine;
      u64 bits = v & 0x1f;                                  // C1, from the value's last character down to its first
      int width = 1;
      for (int64_t q = p - 1; q >= lo; --q) {
        const uint8_t u = (uint8_t)(a.chars[q] - 48);
        if (!continues(u)) break;
        if (width == DEVA_TEXT_MAX_CHARS) {
          flags |= DEVA_TEXT_FLAG_LONG;
          break;
        }
        bits = bits << 5 | (u & 0x1f);
        ++width;
      }
      if (v & 0x10) bits |= ~0ull << (5 * width);
      x[e] = bits;
    }
    // the rank of every value in its mask
    int rank, found;
    block_exclusive(mine, rank_sums, tid, rank, found);
    rank += values;
    // C2: count 0 stands alone; the odd counts are the running sums of the odd values, the even counts from count 2 on
    // those of the even values from value 2 on
    u64 even = 0, odd = 0;
    {
      int j = rank;
#pragma unroll
      for (int e = 0; e < kItems; ++e) {
        if (!is_value[e]) continue;
        if (j & 1) odd += x[e];
        else if (j > 0) even += x[e];
        ++j;
      }
    }
    u64 even_before, even_all, odd_before, odd_all;
    block_exclusive(even, even_sums, tid, even_before, even_all);
    block_exclusive(odd, odd_sums, tid, odd_before, odd_all);
    even = carry_even + even_before;
    odd = carry_odd + odd_before;
    u64 sum = 0;
    {
      int j = rank;
#pragma unroll
      for (int e = 0; e < kItems; ++e) {
        if (!is_value[e]) continue;
        u64 count = x[e];
        if (j & 1) count = odd += x[e];
        else if (j > 0) count = even += x[e];
        if ((long long)count < 0 || (long long)count > a.total) flags |= DEVA_TEXT_FLAG_COUNT;
        x[e] = count;
        sum += count;
        ++j;
      }
    }
    // the starts: s_{j+1} = c_0 + ... + c_j
    u64 start_before, start_all;
    block_exclusive(sum, start_sums, tid, start_before, start_all);
    u64 start = carry_start + start_before;
    {
      int j = rank;
#pragma unroll
      for (int e = 0; e < kItems; ++e) {
        if (!is_value[e]) continue;
        start += x[e];
        const int64_t at = out0 + 1 + j;
        if (at >= 0 && at < a.words_cap) a.runs[at] = (int32_t)start;
        ++j;
      }
    }
    values += found;
    carry_even += even_all;
    carry_odd += odd_all;
    carry_start += start_all;
  }
  if (tid == 0 && (values == 0 || carry_start != (u64)a.total)) flags |= DEVA_TEXT_FLAG_SUM;
  if (flags) atomicOr(reinterpret_cast<u64*>(a.info), (u64)flags);
}

LAUNCH_CHECK_DEFINE_LAUNCHED()

}  // namespace
}  // namespace deva_text

extern "C" int deva_text_encode_count(const int32_t* n_in, const int64_t* base, const int32_t* bounds, int64_t bounds_len, int n,
                                      int height, int width, int32_t* text_len, int64_t* text_base, int64_t* text_total,
                                      const int64_t* first, void* stream) {
  using namespace deva_text;
  struct deva_text_plan plan;
  if (int rc = count_check(n_in, base, bounds, bounds_len, n, height, width, text_len, text_base, text_total, first, &plan)) return rc;
  if (n == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const EncodeArgs a = {n_in, base, bounds, bounds_len, (int64_t)height * width};
  hipLaunchKernelGGL(text_len_kernel, dim3(plan.mask_grid), dim3(kBlock), 0, st, a, text_len);
  hipLaunchKernelGGL(text_base_kernel, dim3(plan.scan_grid), dim3(kBlock), 0, st, text_len, n, first, text_base, text_total);
  return launched("deva_text_encode_count");
}

extern "C" int deva_text_encode_write(const int32_t* n_in, const int64_t* base, const int32_t* bounds, int64_t bounds_len, int n,
                                      int height, int width, const int64_t* text_base, uint8_t* chars, int64_t capacity, void* stream) {
  using namespace deva_text;
  struct deva_text_plan plan;
  if (int rc = write_check(n_in, base, bounds, bounds_len, n, height, width, text_base, chars, capacity, &plan)) return rc;
  if (n == 0 || capacity == 0) return 0;
  const EncodeArgs a = {n_in, base, bounds, bounds_len, (int64_t)height * width};
  hipLaunchKernelGGL(text_write_kernel, dim3(plan.mask_grid), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a, text_base, chars,
                     capacity);
  return launched("deva_text_encode_write");
}

extern "C" int deva_text_parse(const uint8_t* chars, int64_t chars_len, const int64_t* text_first, int n, int height, int width,
                               void* scratch, int64_t scratch_bytes, int32_t* runs, int64_t words_cap, int64_t* info, void* stream) {
  using namespace deva_text;
  struct deva_text_plan plan;
  if (int rc = parse_check(chars, chars_len, text_first, n, height, width, scratch, scratch_bytes, runs, words_cap, info, &plan)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Scratch sc = n ? carve(scratch, n) : Scratch{nullptr, nullptr};
  const ParseArgs a = {chars, text_first, sc.values, sc.flags, runs, info, chars_len, words_cap, (int64_t)height * width, n};
  if (n) hipLaunchKernelGGL(values_kernel, dim3(plan.mask_grid), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(first_kernel, dim3(1), dim3(kBlock), 0, st, a);
  if (n) hipLaunchKernelGGL(starts_kernel, dim3(plan.mask_grid), dim3(kBlock), 0, st, a);
  return launched("deva_text_parse");
}
