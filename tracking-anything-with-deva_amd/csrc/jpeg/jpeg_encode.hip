// deva_jpeg_scan and deva_jpeg_place (include/deva_jpeg.h, rules J1-J10): the entropy-coded data of a baseline JPEG coded
// from an RGB plane on the device.
//
//   transform_kernel  one workgroup per tile of 1024 pixels of one MCU row (64 x 16 at 420, 128 x 8 at 444).  The tile's
//                     rows are staged in LDS from aligned 16-byte pieces (one 16-byte load where the piece lies inside the
//                     row, byte loads at the row's two ends; rows and columns behind the picture repeat the last, J2).
//                     A lane converts four pixels (J1; at 420 a 2 x 2, whose chroma it averages, J3).  The two DCT passes
//                     (J4) take a lane per row, then per column, of every block of the tile; the column's lane quantises
//                     (J5, one exact 32-bit division a coefficient) and leaves int16 in zigzag order in LDS, from where
//                     the tile's blocks, which are consecutive in scan order (J7), leave in 16-byte stores.
//   interval_kernel   one workgroup owns a restart interval (J8) and walks its blocks kBlock a step, a lane per block.
//                     The lane walks its 64 coefficients once for a bit count (J6; the DC predictor is the DC of the
//                     block it names, read from the scratch), a workgroup scan places it, and it walks them again to OR
//                     its codes, most significant bit first, into the bit buffer in LDS: kBlock blocks of at most
//                     kBlockBits bits.  Stuffing (J9) changes the byte count after the bits are placed, so the buffer's
//                     whole bytes go through passes of kStuffBytes, 16 bytes a lane: count the FFs, scan, write the bytes
//                     and their zeros into the stage, whose whole 16-byte chunks leave for the interval's slot.  Bits
//                     short of a byte are carried to the next step's buffer, bytes short of a chunk stay in the stage.
//   offsets_kernel    one workgroup: byte counts -> offsets; info.
//   place_kernel      one workgroup per interval: its slot -> out, behind the intervals before it, below `capacity`.
//
// Every load lies inside the plane or the scratch; every store lies inside the scratch as deva_jpeg_plan sizes it,
// out[0, capacity) and info, at places that depend on sizes and scanned counts alone.
#include <hip/hip_runtime.h>

#include "../block_scan.h"
#include "../launch_check.h"
#include "jpeg_plan.h"

namespace deva_jpeg {
namespace {

constexpr int kWaves = kBlock / 64;
constexpr int kWords = kBufferBytes / 4;
constexpr int kChunks = kBufferBytes / 16;
constexpr int kStageChunks = kStageBytes / 16;
static_assert(kBlock == 256 && kWaves == 4, "the lane maps below");
static_assert(15 + 2 * kStuffBytes + 2 <= kStageBytes && kStageBytes % 16 == 0, "a pass's bytes, all stuffed, behind the carried ones; the marker");

using block_scan::block_exclusive;
using block_scan::Sum;

__constant__ HuffmanTables kHuffman = huffman_tables();

struct Unzigzag {
  uint8_t z[64];
};
constexpr Unzigzag unzigzag() {
  Unzigzag u = {};
  for (int z = 0; z < 64; ++z) u.z[kZigzag[z]] = (uint8_t)z;
  return u;
}
__constant__ Unzigzag kUnzigzag = unzigzag();

// ------------------------------------------------------------------------------------------ J1-J5
struct TransformArgs {
  const uint8_t* plane;
  int height, width, mcus_x;
  int16_t* coefs;
  QuantTables q;
};

// The aligned 16-byte pieces that cover the bytes [lo, hi) of the row that begins `row` bytes into the plane (row_bytes
// long) -> `stage`; piece `piece` is this lane's.  `skew` is the plane's address mod 16, so plane byte i lies at address
// skew + i mod 16, and byte 0 of `stage` is plane byte first - skew with first = (skew + row + lo) rounded down to 16.
__device__ __forceinline__ void stage_piece(const uint8_t* plane, int skew, int row, int row_bytes, int lo, int hi, int piece, uint4* stage) {
  const int at = ((skew + row + lo) & ~15) - skew + 16 * piece;     // this piece's first byte in the plane (below `row + lo` at most by 15)
  if (at >= row + hi) return;
  if (at >= row && at + 16 <= row + row_bytes) {
    stage[piece] = *reinterpret_cast<const uint4*>(plane + at);
    return;
  }
  uint8_t* bytes = reinterpret_cast<uint8_t*>(stage + piece);
  for (int b = 0; b < 16; ++b)
    if (at + b >= row && at + b < row + row_bytes) bytes[b] = plane[at + b];
}

__device__ __forceinline__ void convert(const uint8_t* rgb, int& y, int& cb, int& cr) {
  const int r = rgb[0], g = rgb[1], b = rgb[2];
  y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  cb = ((-11059 * r - 21709 * g + 32768 * b + 32767) >> 16) + 128;
  cr = ((32768 * r - 27439 * g - 5329 * b + 32767) >> 16) + 128;
}

template <bool k420>
__global__ __launch_bounds__(kBlock) void transform_kernel(TransformArgs a) {
  constexpr int kMcu = k420 ? 16 : 8, kPer = k420 ? 6 : 3;
  constexpr int kWidth = tile_width(kMcu), kMcus = tile_mcus(kMcu);       // 64 x 16 or 128 x 8 pixels; 4 or 16 MCUs
  constexpr int kPieces = (15 + 3 * kWidth + 15) / 16;                    // 16-byte pieces that cover a row of the tile at any skew
  constexpr int kChromaWidth = k420 ? kWidth / 2 : kWidth;
  constexpr int kTileBlocks = kMcus * kPer;                               // 24 or 48
  static_assert(kMcu * kPieces <= kBlock && kMcu * kWidth == 4 * kBlock, "a lane stages one piece and converts four pixels");
  __shared__ uint4 stage[kMcu * kPieces];
  __shared__ __align__(16) uint8_t luma[kMcu * kWidth];
  __shared__ __align__(16) uint8_t chroma[2][8 * kChromaWidth];
  __shared__ __align__(16) int16_t passed[kTileBlocks * 64];
  __shared__ __align__(16) int16_t coded[kTileBlocks * 64];
  __shared__ uint32_t divisor[2][64];

  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kWidth, y0 = blockIdx.y * kMcu;
  const int row_bytes = 3 * a.width;
  const int skew = (int)(reinterpret_cast<uintptr_t>(a.plane) & 15);
  const int lo = 3 * x0, hi = 3 * min(x0 + kWidth, a.width);               // (x0 < width: a tile begins on an MCU that holds a pixel)
  auto row_of = [&](int r) { return min(y0 + r, a.height - 1) * row_bytes; };   // J2; (the plane has at most 2^29 bytes)
  if (tid < kMcu * kPieces) stage_piece(a.plane, skew, row_of(tid / kPieces), row_bytes, lo, hi, tid % kPieces, stage + (tid / kPieces) * kPieces);
  if (tid < 128) divisor[tid >> 6][tid & 63] = (uint32_t)a.q.q[tid >> 6][tid & 63] << 15;
  __syncthreads();

  const uint8_t* staged = reinterpret_cast<const uint8_t*>(stage);
  auto pixel = [&](int r, int c) {                                         // the staged RGB of row r, column c of the tile
    const int x = min(x0 + c, a.width - 1);                                // J2
    return staged + r * kPieces * 16 + ((skew + row_of(r) + lo) & 15) + 3 * x - lo;
  };
  if constexpr (k420) {
    const int qy = tid >> 5, qx = tid & 31;
    int cb_sum = 2, cr_sum = 2;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 2 * qy + (e >> 1), c = 2 * qx + (e & 1);
      int y, cb, cr;
      convert(pixel(r, c), y, cb, cr);
      luma[r * kWidth + c] = (uint8_t)y;
      cb_sum += cb, cr_sum += cr;
    }
    chroma[0][qy * kChromaWidth + qx] = (uint8_t)(cb_sum >> 2);            // J3
    chroma[1][qy * kChromaWidth + qx] = (uint8_t)(cr_sum >> 2);
  } else {
    const int r = tid >> 5;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 4 * (tid & 31) + e;
      int y, cb, cr;
      convert(pixel(r, c), y, cb, cr);
      luma[r * kWidth + c] = (uint8_t)y;
      chroma[0][r * kWidth + c] = (uint8_t)cb;
      chroma[1][r * kWidth + c] = (uint8_t)cr;
    }
  }
  __syncthreads();

  const int mcu0 = blockIdx.x * kMcus;
  const int blocks = min(kMcus, a.mcus_x - mcu0) * kPer;
  // J4, rows: |sum| < 2^22
  for (int item = tid; item < 8 * blocks; item += kBlock) {
    const int b = item >> 3, r = item & 7, i = b / kPer, j = b % kPer;
    const uint8_t* samples;
    if constexpr (k420) samples = j < 4 ? luma + (8 * (j >> 1) + r) * kWidth + 16 * i + 8 * (j & 1) : chroma[j - 4] + r * kChromaWidth + 8 * i;
    else samples = (j == 0 ? luma : chroma[j - 1]) + r * kWidth + 8 * i;
    const uint2 packed = *reinterpret_cast<const uint2*>(samples);
    int x[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) x[n] = (int)(((n < 4 ? packed.x : packed.y) >> (8 * (n & 3))) & 255) - 128;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      int sum = 1024;
#pragma unroll
      for (int n = 0; n < 8; ++n) sum += kDct[k][n] * x[n];
      passed[b * 64 + r * 8 + k] = (int16_t)(sum >> 11);
    }
  }
  __syncthreads();
  // J4, columns: |u| < 2^28; J5
  for (int item = tid; item < 8 * blocks; item += kBlock) {
    const int b = item >> 3, c = item & 7, j = b % kPer;
    const int table = (k420 ? j >= 4 : j >= 1) ? 1 : 0;
    int t[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) t[r] = passed[b * 64 + r * 8 + c];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      int u = 0;
#pragma unroll
      for (int r = 0; r < 8; ++r) u += kDct[k][r] * t[r];
      const uint32_t d = divisor[table][8 * k + c];                        // Q << 15
      const uint32_t level = ((uint32_t)abs(u) + (d >> 1)) / d;
      coded[b * 64 + kUnzigzag.z[8 * k + c]] = (int16_t)(u < 0 ? -(int)level : (int)level);
    }
  }
  __syncthreads();
  uint4* out = reinterpret_cast<uint4*>(a.coefs + ((int64_t)blockIdx.y * a.mcus_x + mcu0) * kPer * 64);
  const uint4* in = reinterpret_cast<const uint4*>(coded);
  for (int piece = tid; piece < 8 * blocks; piece += kBlock) out[piece] = in[piece];
}

// ------------------------------------------------------------------------------------------ J6-J9
struct IntervalArgs {
  const int16_t* coefs;
  int64_t* sizes;
  uint8_t* slots;
  int64_t slot_bytes;
  int mcus, restart, per, intervals;
};

// J6 on one block: emit(value, bits) for every code word with its extra bits behind it, in stream order; 1 <= bits <= 26
template <typename Emit>
__device__ __forceinline__ void code_block(const int16_t* coef, int predictor, const uint32_t* ac, const uint32_t* dc, Emit&& emit) {
  const uint4* pieces = reinterpret_cast<const uint4*>(coef);
  auto word = [&](int value, uint32_t entry) {
    const int size = 32 - __clz(abs(value));                               // 0 for 0; at most 11 (DC) and 10 (AC) by J4's bounds, 16 by the type
    const uint32_t extra = (uint32_t)(value >= 0 ? value : value + (1 << size) - 1);
    emit((entry & 0xffffu) << size | extra, (int)(entry >> 16) + size);
  };
  int run = 0;
  // (neither loop is unrolled: every unrolled copy of the divergent body holds exec masks in SGPRs, and 64 of them spill)
#pragma unroll 1
  for (int p = 0; p < 8; ++p) {
    const uint4 v = pieces[p];
    if (p > 0 && (v.x | v.y | v.z | v.w) == 0) {
      run += 8;
      continue;
    }
    unsigned long long low = (unsigned long long)v.y << 32 | v.x, high = (unsigned long long)v.w << 32 | v.z;
#pragma unroll 1
    for (int e = 0; e < 8; ++e) {
      const int value = (int)(int16_t)(uint16_t)low;
      low = low >> 16 | high << 48, high >>= 16;
      if (p == 0 && e == 0) {
        const int diff = value - predictor;
        word(diff, dc[(32 - __clz(abs(diff))) & 15]);
        continue;
      }
      if (value == 0) {
        ++run;
        continue;
      }
      for (; run > 15; run -= 16) emit(ac[0xF0] & 0xffffu, (int)(ac[0xF0] >> 16));      // ZRL
      word(value, ac[(run << 4 | (32 - __clz(abs(value)))) & 255]);
      run = 0;
    }
  }
  if (run > 0) emit(ac[0] & 0xffffu, (int)(ac[0] >> 16));                                // EOB
}

// `value` (below 2^n, 1 <= n <= 27) ORed into the buffer at bit `at`, most significant bit first; nothing beyond the buffer
__device__ __forceinline__ void put(uint32_t* buffer, uint32_t at, uint32_t value, int n) {
  const uint32_t word = at >> 5, shift = at & 31;
  const unsigned long long window = (unsigned long long)value << (64 - (int)shift - n);
  if (word < (uint32_t)kWords) atomicOr(&buffer[word], (uint32_t)(window >> 32));
  if ((uint32_t)window != 0 && word + 1 < (uint32_t)kWords) atomicOr(&buffer[word + 1], (uint32_t)window);
}

__global__ __launch_bounds__(kBlock) void interval_kernel(IntervalArgs a) {
  __shared__ uint4 buffer4[kChunks];
  __shared__ uint4 stage4[kStageChunks];
  __shared__ uint32_t tables[2 * 256 + 2 * 16];
  __shared__ uint32_t parts[kWaves];
  uint32_t* buffer = reinterpret_cast<uint32_t*>(buffer4);
  uint8_t* stage = reinterpret_cast<uint8_t*>(stage4);
  const int tid = threadIdx.x, interval = blockIdx.x;
  const int mcu0 = interval * a.restart, mcu1 = min(mcu0 + a.restart, a.mcus);
  const int first = mcu0 * a.per, count = (mcu1 - mcu0) * a.per;          // (at most 2^22 blocks in all)
  uint8_t* slot = a.slots + (int64_t)interval * a.slot_bytes;
  const bool k420 = a.per == 6;

  for (int w = tid; w < kWords; w += kBlock) buffer[w] = 0;
  for (int e = tid; e < 2 * 256 + 2 * 16; e += kBlock) tables[e] = kHuffman.entry[e];
  __syncthreads();

  uint32_t pending = 0;     // bits short of a byte at the buffer's front, from the step before (uniform over the workgroup, as all below)
  uint32_t fill = 0;        // bytes short of a chunk at the stage's front
  int64_t written = 0;      // bytes of the slot stored so far: whole chunks

  for (int begin = 0; begin < count; begin += kBlock) {
    const int b = begin + tid;
    const bool live = b < count;
    const int g = first + b, m = g / a.per, j = g - m * a.per;
    const bool chrominance = k420 ? j >= 4 : j >= 1;
    const int16_t* coef = a.coefs + (int64_t)g * 64;
    const uint32_t* ac = tables + (chrominance ? 256 : 0);
    const uint32_t* dc = tables + 512 + (chrominance ? 16 : 0);
    int predictor = 0;                                                     // J6, J8: the previous block of the component within the interval
    if (live) {
      if (k420 && j >= 1 && j < 4) predictor = coef[-64];
      else if (m > mcu0) predictor = coef[k420 && j == 0 ? -3 * 64 : -a.per * 64];
    }
    // one text of J6 for both walks (two inlined copies of it cost more SGPRs than the kernel has): the first counts the
    // block's bits, the scan places it, the second ORs its codes into the buffer
    uint32_t at = 0, all = 0;
#pragma unroll 1
    for (int walk = 0; walk < 2; ++walk) {
      if (live)
        code_block(coef, predictor, ac, dc, [&](uint32_t value, int n) {
          if (walk) put(buffer, at, value, n);
          at += (uint32_t)n;
        });
      if (walk == 0) {
        uint32_t before;
        block_exclusive<Sum>(at, 0u, parts, tid, before, all);
        at = pending + before;
      }
    }
    uint32_t total = pending + all;
    const bool last = begin + kBlock >= count;
    if (last) {                                                            // J8: 1-bits up to the byte
      const uint32_t pad = (0u - total) & 7;
      if (tid == 0 && pad) put(buffer, total, (1u << pad) - 1, (int)pad);
      total += pad;
    }
    __syncthreads();                                                       // every code of the step is in the buffer
    const uint32_t bytes = total >> 3;
    // J9 over the buffer's whole bytes
    for (uint32_t pass = 0; pass < bytes; pass += kStuffBytes) {
      const uint4 piece = buffer4[(pass >> 4) + tid];
      const int valid = min(max((int)bytes - (int)pass - 16 * tid, 0), 16);
      // the piece's bytes in stream order, most significant first; those behind `valid` cleared, so none of them is FF
      unsigned long long high = (unsigned long long)piece.x << 32 | piece.y, low = (unsigned long long)piece.z << 32 | piece.w;
      if (valid <= 8) low = 0, high = valid ? high & ~0ull << (64 - 8 * valid) : 0;
      else if (valid < 16) low &= ~0ull << (128 - 8 * valid);
      auto full_bytes = [](unsigned long long v) {                         // how many of the eight bytes are FF
        v &= v >> 1, v &= v >> 2, v &= v >> 4;
        return (uint32_t)__popcll(v & 0x0101010101010101ull);
      };
      const uint32_t mine = (uint32_t)valid + full_bytes(high) + full_bytes(low);
      uint32_t stuffed_before, stuffed;
      block_exclusive<Sum>(mine, 0u, parts, tid, stuffed_before, stuffed);
      uint32_t at = fill + stuffed_before;                                 // at + mine <= 15 + 2 * kStuffBytes
#pragma unroll 1
      for (int e = 0; e < valid; ++e) {
        const uint32_t byte = (uint32_t)(high >> 56);
        high = high << 8 | low >> 56, low <<= 8;
        stage[at++] = (uint8_t)byte;
        if (byte == 0xFF) stage[at++] = 0;
      }
      __syncthreads();
      fill += stuffed;
      const uint32_t chunks = fill >> 4;
      for (uint32_t c = tid; c < chunks; c += kBlock) {
        const int64_t to = written + 16 * (int64_t)c;
        if (to + 16 <= a.slot_bytes) *reinterpret_cast<uint4*>(slot + to) = stage4[c];
      }
      uint4 keep = make_uint4(0, 0, 0, 0);
      if (tid == 0 && chunks) keep = stage4[chunks];                       // (chunks < kStageChunks: fill < kStageBytes - 16)
      __syncthreads();
      if (tid == 0 && chunks) stage4[0] = keep;
      written += 16 * (int64_t)chunks;
      fill &= 15;
      __syncthreads();
    }
    // the bits short of a byte go to the front of the next step's buffer
    const uint32_t rest = total & 7;                                       // (0 behind the last step)
    const uint32_t carried = rest ? (buffer[bytes >> 2] >> (24 - 8 * (bytes & 3))) & 255 : 0;
    __syncthreads();
    for (uint32_t w = tid; w < min((total >> 5) + 2, (uint32_t)kWords); w += kBlock) buffer[w] = 0;
    __syncthreads();
    if (tid == 0 && rest) buffer[0] = carried << 24;
    pending = rest;                                                        // (the scan's barriers stand between this store and the next step's codes)
  }
  // J8: the marker behind every interval but the last; what waits in the stage
  const bool marker = interval + 1 < a.intervals;
  if (tid == 0 && marker) stage[fill] = 0xFF, stage[fill + 1] = (uint8_t)(0xD0 + (interval & 7));
  if (marker) fill += 2;
  __syncthreads();
  const int64_t to = written + 16 * (int64_t)tid;
  if ((uint32_t)tid < (fill + 15) >> 4 && to + 16 <= a.slot_bytes) *reinterpret_cast<uint4*>(slot + to) = stage4[tid];
  if (tid == 0) a.sizes[interval] = written + fill;
}

// ------------------------------------------------------------------------------------------ offsets, info
struct PlaceArgs {
  const int64_t* sizes;
  int64_t* offsets;
  const uint8_t* slots;
  int64_t slot_bytes;
  uint8_t* out;
  int64_t capacity;
  int64_t* info;
  int intervals, blocks;
};

__global__ __launch_bounds__(kBlock) void offsets_kernel(PlaceArgs a) {
  __shared__ long long parts[kWaves];
  const int tid = threadIdx.x;
  long long running = 0;
  for (int begin = 0; begin < a.intervals; begin += kBlock) {
    const int s = begin + tid;
    const bool live = s < a.intervals;
    long long before, all;
    block_exclusive<Sum>(live ? (long long)a.sizes[s] : 0ll, 0ll, parts, tid, before, all);
    if (live) a.offsets[s] = running + before;
    running += all;
  }
  if (tid == 0) {
    a.info[0] = running;
    a.info[1] = a.blocks;
    a.info[2] = running > a.capacity ? 1 : 0;
    a.info[3] = a.intervals;
  }
}

__global__ __launch_bounds__(kBlock) void place_kernel(PlaceArgs a) {
  const int tid = threadIdx.x, s = blockIdx.x;
  const int64_t at = a.offsets[s];
  const int64_t bytes = min(a.sizes[s], a.capacity - at);
  const uint8_t* slot = a.slots + (int64_t)s * a.slot_bytes;
  for (int64_t i = tid; i < bytes; i += kBlock) a.out[at + i] = slot[i];
}

LAUNCH_CHECK_DEFINE_LAUNCHED()

void place(const struct deva_jpeg_plan& plan, const Scratch& sc, uint8_t* out, int64_t capacity, int64_t* info, hipStream_t st) {
  const PlaceArgs p = {sc.sizes, sc.offsets, sc.slots, plan.slot_bytes, out, capacity, info, plan.intervals, plan.blocks};
  hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(kBlock), 0, st, p);
  if (capacity > 0) hipLaunchKernelGGL(place_kernel, dim3(plan.intervals), dim3(kBlock), 0, st, p);
}

}  // namespace
}  // namespace deva_jpeg

extern "C" int deva_jpeg_scan(const uint8_t* plane, int height, int width, int quality, int subsampling, int restart, void* scratch,
                              int64_t scratch_bytes, uint8_t* out, int64_t capacity, int64_t* info, void* stream) {
  using namespace deva_jpeg;
  struct deva_jpeg_plan plan;
  if (int rc = scan_check(plane, height, width, quality, subsampling, restart, scratch, scratch_bytes, out, capacity, info, &plan)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Scratch sc = carve(scratch, plan);
  const TransformArgs t = {plane, height, width, plan.mcus_x, sc.coefs, quant_tables(quality)};
  const int tiles = (plan.mcus_x + tile_mcus(plan.mcu) - 1) / tile_mcus(plan.mcu);
  if (subsampling == DEVA_JPEG_420) hipLaunchKernelGGL(transform_kernel<true>, dim3(tiles, plan.mcus_y), dim3(kBlock), 0, st, t);
  else hipLaunchKernelGGL(transform_kernel<false>, dim3(tiles, plan.mcus_y), dim3(kBlock), 0, st, t);
  const IntervalArgs a = {sc.coefs, sc.sizes, sc.slots, plan.slot_bytes, plan.mcus_x * plan.mcus_y, plan.restart, plan.blocks_per_mcu, plan.intervals};
  hipLaunchKernelGGL(interval_kernel, dim3(plan.intervals), dim3(kBlock), 0, st, a);
  place(plan, sc, out, capacity, info, st);
  return launched("deva_jpeg_scan");
}

extern "C" int deva_jpeg_place(int height, int width, int subsampling, int restart, void* scratch, int64_t scratch_bytes, uint8_t* out,
                               int64_t capacity, int64_t* info, void* stream) {
  using namespace deva_jpeg;
  struct deva_jpeg_plan plan;
  if (int rc = place_check("deva_jpeg_place", height, width, subsampling, restart, scratch, scratch_bytes, out, capacity, info, &plan)) return rc;
  place(plan, carve(scratch, plan), out, capacity, info, static_cast<hipStream_t>(stream));
  return launched("deva_jpeg_place");
}
