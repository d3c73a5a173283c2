// Host side of the JPEG coder (jpeg_encode.hip): every argument check of deva_jpeg_scan and deva_jpeg_place, the MCU and
// interval geometry, the scratch layout, the capacity sizes that deva_jpeg_plan exposes, and the tables of ITU-T T.81
// Annex K with what rules J4-J6 derive from them at compile time.  No HIP in here: jpeg_plan.cpp builds with the host
// compiler alone (tests/jpeg_plan_sanitize_main.cpp runs it under the host sanitizers).
#pragma once
#include <stdint.h>

#include "../host_args.h"
#include "deva_jpeg.h"

namespace deva_jpeg {
using namespace host_args;

constexpr int kBlock = 256;                          // lanes of a workgroup: 4 waves; an interval's workgroup codes kBlock blocks a step
constexpr int kBlockBits = 20 + 63 * 26;             // J6: a DC code of 9 + 11 bits, 63 AC codes of 16 + 10 bits
constexpr int kBufferBytes = 53248;                  // the bit buffer of a step: kBlock blocks, 7 bits carried in, 7 of padding
constexpr int kStuffBytes = 4096;                    // bytes of the bit buffer one stuffing pass takes: 16 a lane
constexpr int kStageBytes = 2 * kStuffBytes + 32;    // the stuffed bytes of a pass behind at most 15 carried ones; the marker
constexpr int kTableBytes = (2 * 256 + 2 * 16) * 4;  // the four Huffman tables in LDS
constexpr int kLdsBytes = kBufferBytes + kStageBytes + kTableBytes + 64;
static_assert(kBufferBytes * 8 >= kBlock * kBlockBits + 14 && kBufferBytes % kStuffBytes == 0, "a step's bits fit the buffer");
static_assert(kStuffBytes == 16 * kBlock, "a lane takes one 16-byte piece of the bit buffer in a stuffing pass");
static_assert(kLdsBytes <= 65536, "static LDS of a workgroup");

// the transform's tile: 1024 pixels of one MCU row, a lane per 2 x 2 (420) or per 1 x 4 (444)
constexpr int kTilePixels = 1024;
constexpr int tile_width(int mcu) { return kTilePixels / mcu; }        // 64 at 420, 128 at 444
constexpr int tile_mcus(int mcu) { return tile_width(mcu) / mcu; }     // 4 at 420, 16 at 444

void set_error(const char* fmt, ...);  // jpeg_plan.cpp; text behind deva_jpeg_last_error()
const char* last_error();

#define DEVA_JPEG_REQUIRE(cond, ...) HOST_ARGS_REQUIRE(deva_jpeg::set_error, cond, __VA_ARGS__)

// ------------------------------------------------------------------------------------------ Annex K
constexpr uint8_t kLuminance[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24,  40,  57,
                                    69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35,  55,  64,
                                    81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kChrominance[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                      99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// kZigzag[z]: the natural index (row * 8 + column) of the z-th coefficient of the scan
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// K.3: how many codes of each length 1 .. 16, and the symbols in code order
constexpr uint8_t kDcCounts[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kAcCounts[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcSymbols[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// Annex C: the canonical codes.  An entry is code | bits << 16; 0 where the table has no code for the symbol.
// Layout: [0, 256) AC luminance, [256, 512) AC chrominance, [512, 528) DC luminance, [528, 544) DC chrominance.
struct HuffmanTables {
  uint32_t entry[2 * 256 + 2 * 16];
};
constexpr HuffmanTables huffman_tables() {
  HuffmanTables t = {};
  for (int chroma = 0; chroma < 2; ++chroma) {
    uint32_t value = 0;
    int k = 0;
    for (int length = 1; length <= 16; ++length) {
      for (int c = 0; c < kAcCounts[chroma][length - 1]; ++c) t.entry[256 * chroma + kAcSymbols[chroma][k++]] = value++ | (uint32_t)length << 16;
      value <<= 1;
    }
    value = 0, k = 0;
    for (int length = 1; length <= 16; ++length) {
      for (int c = 0; c < kDcCounts[chroma][length - 1]; ++c) t.entry[512 + 16 * chroma + k++] = value++ | (uint32_t)length << 16;   // (the DC symbols are 0 .. 11 in order)
      value <<= 1;
    }
  }
  return t;
}
static_assert(huffman_tables().entry[0x00] == (0xAu | 4u << 16) && huffman_tables().entry[0xF0] == (0x7F9u | 11u << 16), "K.5: EOB 1010, ZRL 11111111001");
static_assert(huffman_tables().entry[256 + 0xF0] == (0x3FAu | 10u << 16) && huffman_tables().entry[512 + 11] == (0x1FEu | 9u << 16), "K.6, K.3");
static_assert(sizeof(HuffmanTables) == kTableBytes, "the tables in LDS");

// J4: M[k][n] = round(8192 s_k cos((2n + 1) k pi / 16)); the rows are +- of eight numbers
constexpr int kDct[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},     {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                            {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784}, {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                            {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                            {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567}, {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};
constexpr int64_t dct_row_sum() {
  int64_t worst = 0;
  for (int k = 0; k < 8; ++k) {
    int64_t sum = 0;
    for (int n = 0; n < 8; ++n) sum += kDct[k][n] < 0 ? -kDct[k][n] : kDct[k][n];
    worst = sum > worst ? sum : worst;
  }
  return worst;
}
static_assert(dct_row_sum() * 128 + 1024 < (1 << 22), "J4: the row pass fits in int32 with room");
static_assert(dct_row_sum() * (((dct_row_sum() * 128 + 1024) >> 11) + 1) < (1 << 28), "J4: the column pass stays below 2^28");
static_assert((1ll << 28) + (255ll << 14) < (1ll << 32), "J5: |u| + (Q << 14) fits in uint32");

// J5: Q of `quality` for an Annex K base value
constexpr int quant(int base, int quality) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int q = (base * s + 50) / 100;
  return q < 1 ? 1 : (q > 255 ? 255 : q);
}

// what the kernels take by value: Q in natural order, luminance then chrominance
struct QuantTables {
  uint8_t q[2][64];
};
inline QuantTables quant_tables(int quality) {
  QuantTables t;
  for (int i = 0; i < 64; ++i) t.q[0][i] = (uint8_t)quant(kLuminance[i], quality), t.q[1][i] = (uint8_t)quant(kChrominance[i], quality);
  return t;
}

// ------------------------------------------------------------------------------------------ sizes
// J8 / J10: the bytes of an interval of `blocks` blocks at most: every block at kBlockBits, padded to a byte, every byte
// stuffed, and the marker behind it
inline int64_t interval_worst(int64_t blocks) { return 2 * ((blocks * kBlockBits + 7) / 8) + 2; }

// the scratch of one call, front to back, every piece on a 256-byte boundary
struct Scratch {
  int64_t* sizes;     // [intervals] bytes of every interval, its marker included
  int64_t* offsets;   // [intervals] where every interval begins in the data
  int16_t* coefs;     // [blocks][64] in zigzag order, blocks in scan order
  uint8_t* slots;     // [intervals][slot_bytes]
};
inline int64_t scratch_layout(const struct deva_jpeg_plan& plan, int64_t (&at)[4]) {
  ScratchLayout lay;
  at[0] = lay.take(8ll * plan.intervals);
  at[1] = lay.take(8ll * plan.intervals);
  at[2] = lay.take(plan.coef_bytes);
  at[3] = lay.take(plan.slot_bytes * plan.intervals);
  return lay.at;
}
inline Scratch carve(void* scratch, const struct deva_jpeg_plan& plan) {
  int64_t at[4];
  scratch_layout(plan, at);
  uint8_t* base = static_cast<uint8_t*>(scratch);
  return {reinterpret_cast<int64_t*>(base + at[0]), reinterpret_cast<int64_t*>(base + at[1]), reinterpret_cast<int16_t*>(base + at[2]),
          base + at[3]};
}

// the sizes alone (J1, J8) -> 0 and *plan, or 2 with the text set
int jpeg_plan(const char* what, int height, int width, int subsampling, int restart, struct deva_jpeg_plan* plan);

// every check of deva_jpeg_place, before any launch -> 0 and *plan, or 2 with the text set
int place_check(const char* what, int height, int width, int subsampling, int restart, const void* scratch, int64_t scratch_bytes,
                const uint8_t* out, int64_t capacity, const int64_t* info, struct deva_jpeg_plan* plan);

// every check of deva_jpeg_scan
int scan_check(const uint8_t* plane, int height, int width, int quality, int subsampling, int restart, const void* scratch,
               int64_t scratch_bytes, const uint8_t* out, int64_t capacity, const int64_t* info, struct deva_jpeg_plan* plan);

}  // namespace deva_jpeg
