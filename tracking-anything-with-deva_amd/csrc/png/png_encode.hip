// deva_png_deflate and deva_png_place (include/deva_png.h, rules Z1-Z8): the zlib stream of a PNG file coded from a byte
// plane on the device.
//
//   segment_kernel  one workgroup owns a segment (Z5).  It walks the row strings of its rows DEVA_PNG_STEP bytes a step,
//                   kItems consecutive bytes a lane.  The step's window of the row and of the row above is staged in LDS
//                   from aligned 16-byte pieces (one 16-byte load where the piece lies inside the row, byte loads at the
//                   row's two ends), with two bytes before the step and one behind it, so every lane sees whether a run
//                   starts or ends at each of its bytes.  A run is coded by the lane that holds its LAST byte: a max-scan
//                   of the start positions (plus the start carried from the steps before, a register that is uniform
//                   over the workgroup) gives its length, Z3 and Z4 give its bit count in closed form, a sum-scan of the
//                   bit counts plus the carried bit position places it, and its codes are ORed into a bit buffer in LDS.
//                   The buffer's whole 16-byte chunks leave for the segment's slot with 16-byte stores when it is more
//                   than half full, and at the end.  The two Adler sums of the segment are exact 64-bit integers,
//                   reduced mod 65521 once.
//   offsets_kernel  one workgroup: byte counts -> offsets; the Adler sums of the segments combined; info, 78 01 and the
//                   six trailing bytes.
//   place_kernel    one workgroup per segment: its slot -> out, behind the segments before it, below `capacity`.
//
// The bit buffer: a step adds at most the codes of 1023 bytes of its own at 9 bits and of one run carried in, whose length
// is at most DEVA_PNG_MAX_SIDE * 3 + 1 (a literal, 190 matches of 13 bits, one of 18): fewer than kStepBits bits with
// the block header and the segment's tail.  It is drained when more than kBufferBytes * 8 - kStepBits bits wait in it.
//
// Every load lies inside the plane; every store lies inside the scratch as deva_png_plan sizes it, out[0, capacity) and
// info, at places that depend on sizes and scanned counts alone.
#include <hip/hip_runtime.h>

#include "../block_scan.h"
#include "../launch_check.h"
#include "png_plan.h"

namespace deva_png {
namespace {

static_assert(kBlock == 256 && kItems == 4 && kItems * kBlock == DEVA_PNG_STEP, "the walk's step");
constexpr int kWaves = kBlock / 64;
constexpr int kWords = kBufferBytes / 4;
constexpr int kChunks = kBufferBytes / 16;
constexpr int kStepBits = 12288;
constexpr int kPieces = kStageBytes / 16;
constexpr uint32_t kAdler = 65521;
static_assert(kChunks <= kBlock && kWords % kBlock == 0, "a lane drains one chunk and clears kWords / kBlock words");
static_assert(kBufferBytes * 8 >= 2 * kStepBits, "the buffer takes a step's bits behind what may wait in it");
static_assert(9 * 1023 + 9 + 13 * ((DEVA_PNG_MAX_SIDE * 3) / 258) + 18 + 3 + 7 + 3 + 7 + 32 < kStepBits, "the bits of a step");
static_assert(kStageBytes % 16 == 0 && kStageBytes >= 15 + DEVA_PNG_STEP + 3 + 15 && 2 * kPieces <= kBlock, "the staged window");
typedef unsigned long long u64;

using block_scan::block_exclusive;
using block_scan::Max;
using block_scan::Sum;

// ------------------------------------------------------------------------------------------ Z3 / Z4
__device__ __forceinline__ int literal_bits(int b) { return b < 144 ? 8 : 9; }

// the length symbol of a match of `len` (3 .. 258): its code's bits, the code, the extra bits and their count
__device__ __forceinline__ void length_code(int len, int& code_bits, uint32_t& code, int& extra_bits, uint32_t& extra) {
  int symbol;
  if (len == 258) {
    symbol = 285, extra_bits = 0, extra = 0;
  } else {
    const int l = len - 3;
    if (l < 8) {
      symbol = 257 + l, extra_bits = 0, extra = 0;
    } else {
      extra_bits = 29 - __clz(l);                          // floor(log2(l)) - 2: 1 .. 5
      symbol = 261 + 4 * extra_bits + ((l >> extra_bits) & 3);
      extra = (uint32_t)l & ((1u << extra_bits) - 1);
    }
  }
  if (symbol < 280) code_bits = 7, code = (uint32_t)(symbol - 256);
  else code_bits = 8, code = (uint32_t)(0xC0 + symbol - 280);
}

__device__ __forceinline__ int match_bits(int len) {
  int code_bits, extra_bits;
  uint32_t code, extra;
  length_code(len, code_bits, code, extra_bits, extra);
  return code_bits + extra_bits + 5;
}

// Z3: the bits of a run of `len` bytes of value b
__device__ __forceinline__ uint32_t run_bits(int b, int len) {
  const int lit = literal_bits(b), full = (len - 1) / 258, rest = (len - 1) % 258;
  return (uint32_t)(lit + 13 * full + (rest >= 3 ? match_bits(rest) : rest * lit));
}

// `bits` (LSB first, below 2^n, n <= 24) ORed into the buffer at bit `at`; nothing beyond the buffer
__device__ __forceinline__ void put(uint32_t* buffer, uint32_t at, uint32_t bits, int n) {
  const uint32_t word = at >> 5, shift = at & 31;
  if (word < (uint32_t)kWords) atomicOr(&buffer[word], bits << shift);
  if (shift + n > 32 && word + 1 < (uint32_t)kWords) atomicOr(&buffer[word + 1], bits >> (32 - shift));
}

__device__ __forceinline__ uint32_t put_literal(uint32_t* buffer, uint32_t at, int b) {
  const int n = literal_bits(b);
  const uint32_t code = b < 144 ? 0x30u + b : 0x190u + (b - 144);
  put(buffer, at, __brev(code) >> (32 - n), n);
  return at + n;
}

__device__ __forceinline__ uint32_t put_match(uint32_t* buffer, uint32_t at, int len) {
  int code_bits, extra_bits;
  uint32_t code, extra;
  length_code(len, code_bits, code, extra_bits, extra);
  put(buffer, at, (__brev(code) >> (32 - code_bits)) | extra << code_bits, code_bits + extra_bits + 5);   // (distance 1: five zero bits)
  return at + code_bits + extra_bits + 5;
}

__device__ __forceinline__ void put_run(uint32_t* buffer, uint32_t at, int b, int len) {
  at = put_literal(buffer, at, b);
  const int full = (len - 1) / 258, rest = (len - 1) % 258;
  for (int m = 0; m < full; ++m) at = put_match(buffer, at, 258);
  if (rest >= 3) put_match(buffer, at, rest);
  else
    for (int m = 0; m < rest; ++m) at = put_literal(buffer, at, b);
}

// ------------------------------------------------------------------------------------------ segments
struct SegmentArgs {
  const uint8_t* plane;
  int height, row_bytes, rows_per_segment;
  int64_t slot_bytes;
  int64_t* sizes;
  uint32_t* sums;
  uint8_t* slots;
};

// The aligned 16-byte pieces that cover the bytes [lo, hi) of the row that begins `row` bytes into the plane (row_bytes
// long) -> `stage`; piece `piece` is this lane's.  `skew` is the plane's address mod 16, so plane byte i lies at address
// skew + i mod 16, and byte 0 of `stage` is plane byte first - skew with first = (skew + row + lo) rounded down to 16.
__device__ __forceinline__ void stage_piece(const uint8_t* plane, int skew, int row, int row_bytes, int lo, int hi, int piece, uint4* stage) {
  const int at = ((skew + row + lo) & ~15) - skew + 16 * piece;     // this piece's first byte in the plane (below `row` at most by 15)
  if (at >= row + hi) return;
  if (at >= row && at + 16 <= row + row_bytes) {
    stage[piece] = *reinterpret_cast<const uint4*>(plane + at);
    return;
  }
  uint8_t* bytes = reinterpret_cast<uint8_t*>(stage + piece);
  for (int b = 0; b < 16; ++b)
    if (at + b >= row && at + b < row + row_bytes) bytes[b] = plane[at + b];
}

// whole chunks of the buffer -> the slot, and what is left moved to the buffer's front (uniform over the workgroup)
__device__ __forceinline__ void drain(uint4* buffer, uint8_t* slot, int64_t slot_bytes, uint32_t& flushed, uint32_t chunks, int tid) {
  __syncthreads();                                         // every code of the steps so far is in the buffer
  const int64_t at = (int64_t)(flushed >> 3) + 16 * (int64_t)tid;
  if ((uint32_t)tid < chunks && at + 16 <= slot_bytes) *reinterpret_cast<uint4*>(slot + at) = buffer[tid];
  uint4 keep = make_uint4(0, 0, 0, 0);
  if (tid == 0 && chunks < (uint32_t)kChunks) keep = buffer[chunks];
  __syncthreads();
  uint32_t* words = reinterpret_cast<uint32_t*>(buffer);
#pragma unroll
  for (int w = 0; w < kWords / kBlock; ++w) words[tid + w * kBlock] = 0;
  __syncthreads();
  if (tid == 0) buffer[0] = keep;
  __syncthreads();
  flushed += chunks * 128;
}

__global__ __launch_bounds__(kBlock) void segment_kernel(SegmentArgs a) {
  __shared__ uint4 buffer4[kChunks];
  __shared__ uint4 stage_cur[kPieces], stage_up[kPieces];
  __shared__ int max_parts[kWaves];
  __shared__ uint32_t bit_parts[kWaves];
  __shared__ u64 sum_parts[kWaves];
  uint32_t* buffer = reinterpret_cast<uint32_t*>(buffer4);
  const int tid = threadIdx.x, segment = blockIdx.x;
  const int n = a.row_bytes, string = n + 1;
  const int y0 = segment * a.rows_per_segment, y1 = min(y0 + a.rows_per_segment, a.height);
  const uint32_t items = (uint32_t)(y1 - y0) * (uint32_t)string;   // (at most 8 rows of 3 * 16384 + 1 bytes)
  const int skew = (int)(reinterpret_cast<uintptr_t>(a.plane) & 15);
  uint8_t* slot = a.slots + (int64_t)segment * a.slot_bytes;

#pragma unroll
  for (int w = 0; w < kWords / kBlock; ++w) buffer[tid + w * kBlock] = 0;
  __syncthreads();
  if (tid == 0) put(buffer, 0, 2, 3);                       // BFINAL = 0, BTYPE = 01
  uint32_t bit_at = 3, flushed = 0;                         // bits of the segment so far; those that left the buffer
  u64 sum1 = 0, sum2 = 0;

  for (int y = y0; y < y1; ++y) {
    const int row = y * n;                                  // (the plane has at most 2^29 bytes)
    const bool has_up = y > 0;
    int carried_start = 0;                                  // where the run that is open at the step's start began
    for (int begin = 0; begin < string; begin += DEVA_PNG_STEP) {
      // data bytes begin - 2 .. begin + DEVA_PNG_STEP of the row and of the row above (string position q is data byte q - 1)
      const int lo = max(begin - 2, 0), hi = min(begin + DEVA_PNG_STEP, n);
      if (tid < kPieces) stage_piece(a.plane, skew, row, n, lo, hi, tid, stage_cur);
      else if (has_up && tid >= kBlock / 2 && tid < kBlock / 2 + kPieces) stage_piece(a.plane, skew, row - n, n, lo, hi, tid - kBlock / 2, stage_up);
      __syncthreads();
      const uint8_t* cur = reinterpret_cast<const uint8_t*>(stage_cur);   // data byte i of the row is cur[cur_at + i]
      const uint8_t* up = reinterpret_cast<const uint8_t*>(stage_up);
      const int cur_at = ((skew + row + lo) & 15) - lo, up_at = ((skew + row - n + lo) & 15) - lo;
      const int q0 = begin + tid * kItems;
      int v[kItems + 2];                                    // the string's bytes q0 - 1 .. q0 + kItems; -1 outside the string
#pragma unroll
      for (int e = 0; e < kItems + 2; ++e) {
        const int q = q0 - 1 + e;
        v[e] = -1;
        if (q == 0) v[e] = 2;
        else if (q > 0 && q < string) v[e] = (cur[cur_at + q - 1] - (has_up ? up[up_at + q - 1] : 0)) & 255;
      }
      // run starts: the last start of this lane, then of the lanes before
      int last_start = -1;
#pragma unroll
      for (int e = 0; e < kItems; ++e)
        if (v[e + 1] >= 0 && v[e + 1] != v[e]) last_start = q0 + e;
      int start, step_start;
      block_exclusive<Max>(last_start, -1, max_parts, tid, start, step_start);
      start = max(start, carried_start);
      // runs that end here: their bits; the Adler sums
      uint32_t bits[kItems], mine = 0;
      int length[kItems];
#pragma unroll
      for (int e = 0; e < kItems; ++e) {
        const int q = q0 + e, b = v[e + 1];
        bits[e] = 0;
        length[e] = 0;
        if (b < 0) continue;
        if (b != v[e]) start = q;
        if (b != v[e + 2]) {                                // (v is -1 behind the string: the row's last byte ends a run)
          length[e] = q - start + 1;
          bits[e] = run_bits(b, length[e]);
          mine += bits[e];
        }
        const uint32_t index = (uint32_t)(y - y0) * (uint32_t)string + (uint32_t)q;
        sum1 += (u64)b;
        sum2 += (u64)(items - index) * (u64)b;
      }
      uint32_t before, all;
      block_exclusive<Sum>(mine, 0u, bit_parts, tid, before, all);
      uint32_t at = bit_at - flushed + before;
#pragma unroll
      for (int e = 0; e < kItems; ++e) {
        if (length[e] == 0) continue;
        put_run(buffer, at, v[e + 1], length[e]);
        at += bits[e];
      }
      bit_at += all;
      carried_start = max(carried_start, step_start);
      if (bit_at - flushed > (uint32_t)(kBufferBytes * 8 - kStepBits)) drain(buffer4, slot, a.slot_bytes, flushed, (bit_at - flushed) >> 7, tid);
    }
  }
  // end-of-block (seven zero bits), the stored block: 000, zero bits to the byte boundary, 00 00 FF FF
  const uint32_t bytes = (bit_at + 10 + 7) / 8 + 4;
  if (tid == 0) put(buffer, (bytes - 2) * 8 - flushed, 0xffffu, 16);
  drain(buffer4, slot, a.slot_bytes, flushed, (bytes * 8 - flushed + 127) >> 7, tid);

  u64 before, all1, all2;
  block_exclusive<Sum>(sum1, (u64)0, sum_parts, tid, before, all1);
  block_exclusive<Sum>(sum2, (u64)0, sum_parts, tid, before, all2);
  if (tid == 0) {
    a.sizes[segment] = bytes;
    a.sums[2 * segment] = (uint32_t)(all1 % kAdler);
    a.sums[2 * segment + 1] = (uint32_t)(all2 % kAdler);
  }
}

// ------------------------------------------------------------------------------------------ offsets, info, framing
struct PlaceArgs {
  const int64_t* sizes;
  const uint32_t* sums;
  int64_t* offsets;
  const uint8_t* slots;
  int64_t slot_bytes;
  uint8_t* out;
  int64_t capacity;
  int64_t* info;
  int segments, height, rows_per_segment, string;
};

// Adler-32 over the segments: with A the first sum before segment s (1 at the start) and N its bytes of row strings,
// the second sum grows by N * A + sum2[s] and A by sum1[s]
__global__ __launch_bounds__(kBlock) void offsets_kernel(PlaceArgs a) {
  __shared__ u64 parts[kWaves];
  const int tid = threadIdx.x;
  u64 running = 2, first = 1, second = 0;
  for (int begin = 0; begin < a.segments; begin += kBlock) {
    const int s = begin + tid;
    const bool live = s < a.segments;
    u64 before, all;
    block_exclusive<Sum>(live ? (u64)a.sizes[s] : (u64)0, (u64)0, parts, tid, before, all);
    if (live) a.offsets[s] = (int64_t)(running + before);
    running += all;
    block_exclusive<Sum>(live ? (u64)a.sums[2 * s] : (u64)0, (u64)0, parts, tid, before, all);
    if (live) {
      const u64 rows = (u64)(min((s + 1) * a.rows_per_segment, a.height) - s * a.rows_per_segment);
      const u64 count = rows * (u64)a.string % kAdler;
      second += count * ((first + before) % kAdler) + (u64)a.sums[2 * s + 1];
    }
    first += all;
  }
  u64 before, all;
  block_exclusive<Sum>(second, (u64)0, parts, tid, before, all);
  if (tid == 0) {
    const uint32_t adler = (uint32_t)(all % kAdler) << 16 | (uint32_t)(first % kAdler);
    const int64_t total = (int64_t)running + 6;
    a.info[0] = total;
    a.info[1] = (int64_t)adler;
    a.info[2] = total > a.capacity ? 1 : 0;
    a.info[3] = a.segments;
    auto store = [&](int64_t at, uint32_t byte) {
      if (at < a.capacity) a.out[at] = (uint8_t)byte;
    };
    const int64_t end = (int64_t)running;
    store(0, 0x78), store(1, 0x01);
    store(end, 0x03), store(end + 1, 0x00);
    store(end + 2, adler >> 24), store(end + 3, adler >> 16), store(end + 4, adler >> 8), store(end + 5, adler);
  }
}

__global__ __launch_bounds__(kBlock) void place_kernel(PlaceArgs a) {
  const int tid = threadIdx.x, s = blockIdx.x;
  const int64_t at = a.offsets[s];
  const int64_t bytes = min(a.sizes[s], a.capacity - at);   // (at >= 2)
  const uint8_t* slot = a.slots + (int64_t)s * a.slot_bytes;
  for (int64_t i = tid; i < bytes; i += kBlock) a.out[at + i] = slot[i];
}

LAUNCH_CHECK_DEFINE_LAUNCHED()

void place(const struct deva_png_plan& plan, const Scratch& sc, int height, uint8_t* out, int64_t capacity, int64_t* info, hipStream_t st) {
  const PlaceArgs p = {sc.sizes,      sc.sums, sc.offsets, sc.slots, plan.slot_bytes, out, capacity, info, plan.segments, height,
                       plan.rows_per_segment, plan.row_bytes + 1};
  hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(kBlock), 0, st, p);
  if (capacity > 2) hipLaunchKernelGGL(place_kernel, dim3(plan.segments), dim3(kBlock), 0, st, p);
}

}  // namespace
}  // namespace deva_png

extern "C" int deva_png_deflate(const uint8_t* plane, int height, int width, int bpp, void* scratch, int64_t scratch_bytes, uint8_t* out,
                                int64_t capacity, int64_t* info, void* stream) {
  using namespace deva_png;
  struct deva_png_plan plan;
  if (int rc = deflate_check(plane, height, width, bpp, scratch, scratch_bytes, out, capacity, info, &plan)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Scratch sc = carve(scratch, plan);
  const SegmentArgs a = {plane, height, plan.row_bytes, plan.rows_per_segment, plan.slot_bytes, sc.sizes, sc.sums, sc.slots};
  hipLaunchKernelGGL(segment_kernel, dim3(plan.segments), dim3(kBlock), 0, st, a);
  place(plan, sc, height, out, capacity, info, st);
  return launched("deva_png_deflate");
}

extern "C" int deva_png_place(int height, int width, int bpp, void* scratch, int64_t scratch_bytes, uint8_t* out, int64_t capacity,
                              int64_t* info, void* stream) {
  using namespace deva_png;
  struct deva_png_plan plan;
  if (int rc = place_check("deva_png_place", height, width, bpp, scratch, scratch_bytes, out, capacity, info, &plan)) return rc;
  place(plan, carve(scratch, plan), height, out, capacity, info, static_cast<hipStream_t>(stream));
  return launched("deva_png_place");
}
