// deva_rle_decode (include/deva_rle.h, rules D1-D6): COCO run lengths -> byte or float planes, with the nearest resize
// fused in.
//
// A workgroup owns a tile of 64 x 64 output pixels of one mask (a grid-stride loop over mask x tile).
//
//   walk   (the arithmetic is rle_walk.h's) lane = (column of the tile, quarter of its rows).  The lane's source column
//          sx and first source row sy give p = sx * H + sy; one binary search over the mask's starts finds the last run whose start is <= p (D1: among
//          runs that share a start the last one owns the pixel).  Then 16 output rows: p moves down the column, the run
//          index follows while the next start is <= p (the last start is H * W, above every p: no end test), and the
//          byte run & 1 goes into the tile in LDS.  Row r of the tile is stored shifted right by shift(r) elements, the
//          elements its first pixel's address in the output lies above a 16-byte boundary.
//   store  a work item is 16 bytes of a shifted row, so its place in the output is 16-byte aligned by construction and
//          its place in LDS is 16 bytes (uint8) or 4 bytes (float) aligned.  A piece that lies wholly inside the tile's
//          columns leaves as one 16-byte store; the pieces at the ragged ends leave element by element.
//
// Nothing is read back, no workgroup waits on another, and nothing outside [n][OH][OW] is written: a vector store is
// issued only for a piece whose every element is a pixel of the tile.
#include <hip/hip_runtime.h>

#include "../launch_check.h"
#include "rle_plan.h"
#include "rle_walk.h"

namespace deva_rle {
namespace {

static_assert(kTile == 64 && kBlock == 256 && kSegRows == 16, "a lane of the walk takes a column of the tile and 16 of its 64 rows");
static_assert(kPitch % 16 == 0 && kPitch >= kTile + 15, "a row shifted by up to 15 bytes, every row 16-byte aligned in LDS");

struct Args {
  const int* runs;       // first[n + 1], then the starts
  void* out;
  int n, height, width, out_height, out_width, tiles_x, tiles_y;
  float scale_y, scale_x;
};

// the shift of tile row y of the plane at element offset `plane_low` (low word), from column x0 on
template <typename T>
__device__ __forceinline__ int shift_of(uint32_t out_low, uint32_t plane_low, int y, int out_width, int x0) {
  return row_shift(out_low, plane_low + (uint32_t)y * (uint32_t)out_width + (uint32_t)x0, (uint32_t)sizeof(T));
}

__device__ __forceinline__ void store16(uint8_t* dst, const uint8_t* lds) {
  *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(lds);
}
__device__ __forceinline__ void store16(float* dst, const uint8_t* lds) {
  const uint32_t b = *reinterpret_cast<const uint32_t*>(lds);
  *reinterpret_cast<float4*>(dst) =
      make_float4((float)(b & 0xffu), (float)((b >> 8) & 0xffu), (float)((b >> 16) & 0xffu), (float)(b >> 24));
}

template <typename T>
__global__ __launch_bounds__(kBlock) void rle_decode_kernel(Args a) {
  constexpr int E = 16 / (int)sizeof(T);      // elements of a 16-byte piece
  constexpr int kPieces = kTile / E + 1;      // pieces of a shifted row: the shift is below E
  static_assert((kPieces - 1) * E + E <= kPitch, "every piece lies inside its row of the tile");
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTile * kPitch];
  const int tid = threadIdx.x, col = tid % kTile, seg = tid / kTile;
  const int per_plane = a.tiles_x * a.tiles_y;
  const int64_t tiles = (int64_t)a.n * per_plane, out_pixels = (int64_t)a.out_height * a.out_width;
  const int* first = a.runs;
  const int* starts = a.runs + a.n + 1;
  T* out = static_cast<T*>(a.out);
  const uint32_t out_low = (uint32_t)reinterpret_cast<uintptr_t>(a.out);
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {   // (uniform over the workgroup)
    const int k = (int)(t / per_plane), in_plane = (int)(t - (int64_t)k * per_plane);
    const int y0 = in_plane / a.tiles_x * kTile, x0 = in_plane % a.tiles_x * kTile;
    const int th = min(kTile, a.out_height - y0), tw = min(kTile, a.out_width - x0);
    const int64_t plane = k * out_pixels;
    const uint32_t plane_low = (uint32_t)plane;
    // ---- walk
    const int r0 = seg * kSegRows, r1 = min(r0 + kSegRows, th);
    if (col < tw && r0 < r1) {
      const int* s = starts + first[k];
      const int runs_k = first[k + 1] - first[k] - 1;
      const int column = source_index(x0 + col, a.scale_x, a.width) * a.height;
      int p = column + source_index(y0 + r0, a.scale_y, a.height);
      int run = owner(s, runs_k, p), next = s[run + 1];
      for (int r = r0; r < r1; ++r) {
        p = column + source_index(y0 + r, a.scale_y, a.height);
        run = advance(s, run, next, p);
        tile[r * kPitch + shift_of<T>(out_low, plane_low, y0 + r, a.out_width, x0) + col] = (uint8_t)(run & 1);
      }
    }
    __syncthreads();
    // ---- store
    for (int item = tid; item < th * kPieces; item += kBlock) {
      const int r = item / kPieces, u0 = item % kPieces * E;
      const int shift = shift_of<T>(out_low, plane_low, y0 + r, a.out_width, x0);
      const uint8_t* src = tile + r * kPitch + u0;
      T* row = out + plane + (int64_t)(y0 + r) * a.out_width + x0;
      int c0;   // the tile column of the piece's first element
      if (whole_piece(u0, shift, tw, E, c0)) {
        store16(row + c0, src);
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e)
          if (c0 + e >= 0 && c0 + e < tw) row[c0 + e] = (T)src[e];
      }
    }
    __syncthreads();   // the next tile reuses the LDS
  }
}

LAUNCH_CHECK_DEFINE_LAUNCHED()

}  // namespace
}  // namespace deva_rle

extern "C" int deva_rle_decode(const int32_t* runs_host, const int32_t* runs_device, int64_t words, int n, int height, int width,
                               int out_height, int out_width, int dtype, void* out, void* stream) {
  using namespace deva_rle;
  struct deva_rle_plan plan;
  if (int rc = decode_check(runs_host, runs_device, words, n, height, width, out_height, out_width, dtype, out, &plan)) return rc;
  if (n == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Args a = {runs_device, out, n, height, width, out_height, out_width, plan.tiles_x, plan.tiles_y, plan.scale_y, plan.scale_x};
  if (dtype == DEVA_RLE_F32)
    hipLaunchKernelGGL(rle_decode_kernel<float>, dim3(plan.grid), dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL(rle_decode_kernel<uint8_t>, dim3(plan.grid), dim3(kBlock), 0, st, a);
  return launched("deva_rle_decode");
}
