// 3x3 / stride 1 / pad 1 convolutions as Winograd F(2x2, 3x3) on the fp32 matrix pipes (v_mfma_f32_32x32x2_f32).
//
// Why: the fp32 MFMA runs at 1/16 of the f16 rate and is THE bound of the fp32 frame (the five big 3x3 layers of the
// decoder / value encoder are 76 % of the 480p / 5-object frame at 0.86 - 0.87 of the matrix peak: nothing left to
// schedule).  F(2x2, 3x3) computes a 2x2 output tile from 16 instead of 36 multiply-adds per input channel: 2.25x fewer
// MFMAs, with transforms whose constants are 0, +-1, +-1/2.  A quarter of the accumulated terms: the error against fp64 is
// BELOW the direct kernels' on the layer shapes of the network (2.5e-7 - 1.4e-6 of the output range against 4.3e-7 - 4.8e-6;
// bound 2e-5 in tests/test_gpu_a_conv.py).  Unlike on the f16 pipes the transform is cheap here:
// ~40 VALU instructions per 32 MFMAs (2 048 matrix-pipe cycles) and wave.
//
//   Y = A^T [ sum_c (G g_c G^T) .* (B^T d_c B) ] A        per (output channel, 2x2 tile); g 3x3, d the 4x4 input patch
//
// GEMM view: 16 independent GEMMs (one per transform position p = 4 i + l), M = cout, N = tiles (batch-major, row-major
// inside an image), K = input channels.  A workgroup = 8 waves = 64 output channels x 64 tiles; K advances in steps of 8
// channels through two double-buffered LDS tiles (2 x 2 x 32 KB):
//   * transformed weights U (deva_conv_pack_wino: [c/8][p][c%2][cout_pad][c%8/2], i.e. the four k values a lane feeds to the
//     four MFMAs of a position are one 16-byte read) go global -> LDS as they are, by LDS-DMA (buffer_load_dwordx4 ... lds:
//     the tile's image is lane-linear per wave, 64 lanes x 16 bytes = 1 KB contiguous -- no registers, no LDS stores);
//   * activations: thread (channel, tile) loads the 4x4 patch of its tile (four unaligned 16-byte buffer loads from
//     guard-banded inputs; rows outside the image are out-of-range offsets and come back as zeros), applies ReLU-on-load
//     and B^T d B in registers (16 packed additions) and writes the 16 transformed values as [p][k parity][k/2][tile] (a wave
//     = one channel of all 64 tiles: contiguous loads, conflict-free stores; the B fragment of a position is four 4-byte reads);
//   * per position: one ds_read_b128 (A) + two ds_read2st64_b32 (B) + four MFMAs.
// Output stage: the position sums of a (channel, tile) pair sit in ONE lane (same register index of the accumulators):
// A^T M A is additions in registers, then bias / residual / activation and two 8-byte stores per output channel.
#include <cstdlib>
#include <type_traits>

#include "conv_args.h"

namespace deva {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ f32x4 buf_load4(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

// packed fp32 additions, written out: on scalars the compiler prefers 2 x v_add_f32 (and builds shuffled pairs with moves)
__device__ __forceinline__ f32x2 pk_add(f32x2 a, f32x2 b) {
  f32x2 r;
  asm("v_pk_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) {
  f32x2 r;
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

#ifdef DEVA_CONV_PROBES  // timing-only ablations of the K step (results are wrong), DEVA_WINO_ABLATE: 1 staging stores, 2 activation loads, 4 barrier, 8 weight DMA
#define WINO_ABL(bit) (p.ablate & (bit))
#else
#define WINO_ABL(bit) false
#endif

#define SCHED_PIN() __builtin_amdgcn_sched_barrier(0)  // nothing is scheduled across it

constexpr int WM = 64, WN = 64;  // output channels x tiles of a workgroup
constexpr int KC = 8;            // channels per K step
constexpr int TILE_FLOATS = 16 * 2 * 64 * 4;  // one operand tile of a K step: [p][k parity][row / column][4]

template <int N>
__device__ __forceinline__ constexpr std::integral_constant<int, (N ^ 1)> flip_buf(std::integral_constant<int, N>) { return {}; }
__device__ __forceinline__ int flip_buf(int b) { return b ^ 1; }

struct WinoArgs {
  const float* in0;
  const float* in1;
  int64_t bs0, bs1;
  int c0, ctot;
  int H, W;
  int tiles_x, tiles_per_img, n_tiles;  // 2x2 output tiles
  const float* u;  // transformed weights
  const float* bias;
  int cout, cout_pad;
  int relu_in;
  const float* res;
  int64_t res_bs;
  int act;
  float* out;
  int blocks_m;
  int by_tiles;  // grid numbered XCD-major (see the kernel)
  int ablate;    // `make PROBES=1` builds only (DEVA_WINO_ABLATE), 0 otherwise
};


// TWO waves per SIMD (8 waves, 512 threads), and why: a single wave cannot keep the fp32 matrix pipe busy.  A register-only
// stream of v_mfma_f32_32x32x2_f32 from one wave per SIMD measures 0.79 busy (profiles/pmc_r06/effective_clock.json: the
// probe); the first form of this kernel -- 4 waves, each with all SIXTEEN accumulators of its quadrant in 256 AGPRs -- ran at
// exactly that rate with everything but its MFMAs switched off and at 0.58 busy as a whole; the direct kernels (two and more
// waves per SIMD) reach 0.89.  Here the 16 transform positions are split between the two waves of a SIMD: wave (ph, wq)
// holds the EIGHT accumulators of positions 8 ph .. 8 ph + 7 (rows 2 ph, 2 ph + 1 of M) for quadrant wq (32 channels x 32
// tiles) -- 128 accumulator registers + ~85 others.  No operand is read twice (the LDS tiles are indexed by position).
// Measured against the 4-wave form on one box (tools/convlab --wino, us): up_8_4 256 -> 256 at 120x216 x5 725 -> 667 (742 ->
// 675 with a residual, 786 -> 659 with ReLU-on-load), GRU 1024 -> 1536 1 011 -> 925, fuser 512 -> 512 175 -> 161, up_16_8
// 363 -> 315 / 348 -> 319.
// Staging: thread = (ONE channel = wave, tile = lane): four patch rows, 16 packed additions, 16 LDS stores; the weights
// are four LDS-DMA loads per thread and step.  RELU / RES are compile-time: ReLU-on-load is ONE instruction per element
// (median of x, 0, limit: limit = +inf, or 0 for a masked column -- no NaN canonicalisation in front of it as with v_max).
// The K pipeline (what each of its parts bought is measured in ONE lab call against the previous form, `tools/convlab
// --wino_all --check --rounds 7 --spread`, medians in us for up_8_4 256 -> 256 at 120x216 x5 / GRU 1024 -> 1536 at 30x54 x5 /
// fuser 512 -> 512 at 30x54 x5; every form bit-identical to the previous one, d0.0e+00 on all layers):
//   previous form   671 / 917 / 160   run-time LDS buffer index, weights through 16 registers + 4 ds_write_b128, ONE
//                                     activation register set loaded at the top of step s and staged in front of its barrier
//   (1) K loop unrolled by two over compile-time buffers (an exit after either half: odd counts and one step need no
//       second body, the accumulators are never copied): every LDS address is base + immediate, 46 -> 40 VALU per step.
//       Alone 673 / 924 / 161 -- nothing; under (2) + (3) it is worth 3.3 % (658 / 896 / 156 without it): kept.
//   (2) weights by LDS-DMA, issued behind the barrier for the tile TWO steps ahead: 642 / 876 / 152 (-4.4 %).  228 -> 210
//       VGPRs.  The loop's barrier is a raw s_barrier behind `s_waitcnt vmcnt(4) lgkmcnt(0)`: the DMA is the oldest
//       vector-memory operation in flight, the four activation loads behind it stay in flight across the barrier.
//   (3) activations staged BEHIND the barrier (tile s + 2 into the buffers of tile s, from loads issued a step earlier;
//       still one register set: the loads of tile s + 3 go out right after the stores): 638 / 872 / 151 (-0.5 % more; the
//       median lies below the minimum of (2) on every layer).  194 / 198 VGPRs.
//   dropped: waves 0 - 3 staging behind the barrier and waves 4 - 7 in front of it (the stagger): 725 / 966 / 170, 13 %
//       SLOWER than (3) -- both staging bodies in every step, and the late waves' loads are waited for at the next use.
//   not built: a second activation register set (one suffices once the stores come before the re-issue).
// The compiled step IS the designed step only with the schedule pinned (SCHED_PIN = sched_barrier(0) around every fragment
// read group, MFMA group, the barrier and the staging block; check the -S listing, not the source).  Without the pins the
// register allocator folds the two fragment sets into one and the scheduler sinks each read group below the MFMAs in front
// of it: prefetch distance zero, pair 2 behind the barrier, twelve LDS reads drained at the barrier by both waves of a
// SIMD at once.  Pinned: the reads of pair g + 1 go out in front of the 8 MFMAs of pair g into the other set and are
// waited for a whole MFMA group later (lgkmcnt(9) / (7) / (6)), the MFMAs of pair 2 are issued in front of the barrier,
// behind it come the next tile's first fragments, the staging block, then the MFMAs of pair 3.  The barrier's wait is
// the s_waitcnt BUILTIN, not text inside the asm statement: the compiler cannot see a wait in inline assembly and put
// its own lgkmcnt(3) / (1) / (0) in front of the MFMAs of pair 3 -- a wait for the staging stores and the next tile's
// fragments just issued, i.e. one exposed LDS round trip per step exactly where the MFMAs were meant to cover it.
// Loop overhead: the four load offsets of both sources are built once, the descriptor base advances by a scalar add per
// step and the switch from in0 to in1 is a branch taken once (the 5 v_add + 1 v_cndmask and ~13 scalar instructions of
// every step are gone).
// Resources (hipcc -O3, -Rpass-analysis=kernel-resource-usage), previous form -> now: VGPRs 227 / 227 / 230 / 230 -> 194 /
// 194 / 198 / 198 (<RELU, RES> = ff / ft / tf / tt), LDS 131 072 bytes, occupancy 2, no spills, no scratch.  One wave's
// step <false, false>: 32 MFMA, 46 -> 30 VALU (16 v_pk_add, 9 v_cndmask, 5 v_add for the load offsets), 36 -> 32 LDS
// instructions (the 4 ds_write_b128 are gone), 8 VMEM, 19 -> 14 s_waitcnt.  With the pinned schedule, the offsets built
// once and the shared output stage: VGPRs 196 / 212 / 200 / 212 (the residual instances hold 32 residual + 32 exchanged
// values across the output stage; the K loop itself needs 196 / 200), same LDS, occupancy 2, no spills, no scratch, no
// copies of the 128 accumulator registers; a step <false, false> executes 32 MFMA, 24 VALU (16 v_pk_add, 8 v_cndmask),
// 32 LDS, 8 VMEM, 43 -> 30 scalar instructions; no s_waitcnt in front of the MFMAs of pair 3.
// On counters over the 480p / 5-object frame (profiles/r07/pmc/): matrix pipe 0.656 -> 0.688 busy, VALU instructions
// per launch -18.8 %, MFMA instructions and HBM traffic unchanged; bench.py 170.1 -> 175.8 FPS on one box.
// `make PROBES=1`: DEVA_WINO_ABLATE switches parts of the step off for timing (1 staging stores, 2 activation loads, 4
// barrier, 8 weight DMA; results are wrong).  On up_8_4 (probe build 677 us): -13 / -54 / -55 / -28 us, all four -104.
// Output stage, on all eight waves: A^T M A is linear in the rows of M, so each half reduces its own rows to a partial 2x2
// output in registers.  Half ph keeps the accumulator rows 8 ph .. 8 ph + 7 (eight of a lane's sixteen output channels:
// [0, 16) and [32, 48) of the block for ph = 0, the others for ph = 1), hands the partials of the other eight rows over
// through LDS (64 KB, the weight tiles' space, written and read half by each side) and finishes its own: (partial + partial)
// + bias + residual, activation, store -- bit-identical to the form in which the ph = 0 waves did all sixteen rows and the
// ph = 1 waves left after the hand-over (the sum of the two partials is commutative).  Residual and bias of a wave's eight
// channels are fetched together, up front and in front of the hand-over: a load issued between the stores is waited for
// in full (`out` may alias `res`, so the compiler keeps every load behind the stores in front of it -- in the first form
// that was 16 exposed round trips per workgroup, +20 % on a 32-step layer); they stay in flight across the hand-over's
// barrier (raw, lgkmcnt(0) only).  The 32 exchanged partials of a wave are read in one burst behind the barrier (read at
// the use, every one was a round trip of its own), and the activation code and `out` are held in scalar registers (read
// through `p`, the compiler of this form fetches them from the kernel arguments again for every row, each fetch a wait).
// Grid: cout blocks fastest -- the workgroups that share an activation tile run side by side.  Workgroup b runs on XCD b % 8,
// each with its own L2: as it is, XCD x sees the cout blocks = x (mod 8) of EVERY tile block -- 1/8 of the weights, all the
// activations.  Right when the weights are the bigger operand (GRU: 100 MB of U against 33 MB); when the activations are
// (up_8_4: 132 MB against 4 MB) p.by_tiles renumbers the grid so that an XCD gets a contiguous range of TILE blocks with all
// their cout blocks, one after the other: an activation tile enters one L2, not blocks_m of them (1 - 4 %).
template <bool RELU, bool RES>
__global__ __launch_bounds__(512, 1) void conv_wino_kernel(const WinoArgs p) {
  // ONE array, the weight tiles first: their LDS-DMA destinations (the M0 base of a wave's 1 KB) stay below 64 KB
  __shared__ __attribute__((aligned(16))) float smem[4 * TILE_FLOATS];
#define sA(b) (smem + (b) * TILE_FLOATS)
#define sB(b) (smem + (2 + (b)) * TILE_FLOATS)
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  const int wq = wave & 3, ph = wave >> 2;
  const int wm = wq >> 1, wn = wq & 1;
  int lb = blockIdx.x;
  if (p.by_tiles) {
    const int nb = gridDim.x, x = lb & 7, i = lb >> 3;
    lb = x * (nb >> 3) + min(x, nb & 7) + i;
  }
  const int block_m = lb % p.blocks_m, block_n = lb / p.blocks_m;
  const int m0 = block_m * WM, n0 = block_n * WN;

  // ---- activation staging: thread = (channel c8 = wave of the step's eight, tile st = lane)
  const int c8 = wave, st = lane;
  const int sm = c8 >> 1, sh = c8 & 1;  // k index inside the 16-byte weight chunk, k parity (the MFMA's two k values)
  const int64_t HW = (int64_t)p.H * p.W;
  int poff[4];             // byte offsets of the four patch rows inside a step's first channel plane (out of range: zeros)
  int poff_b0, poff_b1;    // batch item + first column inside in0 / in1 (may be -4: the guard band)
  bool lcol, rcol;
  {
    const int n = min(n0 + st, p.n_tiles - 1);
    const int b = n / p.tiles_per_img;
    const int r = n - b * p.tiles_per_img;
    const int ty = r / p.tiles_x, tx = r - ty * p.tiles_x;
    const int y0 = 2 * ty - 1, x0 = 2 * tx - 1;
    lcol = x0 >= 0;
    rcol = x0 + 3 < p.W;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      poff[i] = (unsigned)(y0 + i) < (unsigned)p.H ? (int)(((int64_t)c8 * HW + (int64_t)(y0 + i) * p.W) * 4) : (int)0x80000000;
    poff_b0 = (int)(((int64_t)b * p.bs0 + x0) * 4);
    poff_b1 = (int)(((int64_t)b * p.bs1 + x0) * 4);
  }
  int voff[4], voff1[4];  // the loads' byte offsets from (source - 16 bytes): the current source's, in1's
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    voff1[i] = poff_b1 + 16 + poff[i];
    voff[i] = p.c0 > 0 ? poff_b0 + 16 + poff[i] : voff1[i];
  }
  uintptr_t act_base = reinterpret_cast<uintptr_t>(p.c0 > 0 ? p.in0 : p.in1) - 16;
  int act_s = 0;
  float pinf = __builtin_inff();
  asm("" : "+v"(pinf));  // (a limit the compiler cannot see through: median(x, 0, +inf) folds to a max WITH the canonicalising max in front)
  const float llim = lcol ? __builtin_inff() : 0.0f, rlim = rcol ? __builtin_inff() : 0.0f;
  const int aoff = ((tid >> 6) * p.cout_pad + (tid & 63)) * 16;  // segment (p, k parity) = tid / 64 + 8 i, chunk tid % 64
  const int astride = 8 * p.cout_pad * 16;

  f32x16 acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.0f;

  const int ksteps = p.ctot / KC;
  f32x4 rb[4];
  // weights of step s -> sA(buf).  LDS-DMA: a wave's 64 lanes x 16 bytes land at (wave-uniform base) + lane * 16, which IS
  // the tile's image ((tid + 512 i) * 16 bytes); no registers, no LDS store instructions
  auto load_w = [&](int s, auto bufc) {
    const int buf = bufc;
    if (WINO_ABL(8)) return;
    const float* ub = p.u + ((int64_t)s * 32 * p.cout_pad + m0) * 4;
    const __amdgpu_buffer_rsrc_t ru = make_rsrc(ub, 0x7fffffff);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ru, (__attribute__((address_space(3))) void*)(sA(buf) + (wave * 64 + 512 * i) * 4), 16, aoff,
                                               i * astride, 0, 0);
  };
  // Activation loads of step s.  The four row offsets of BOTH sources are built once (voff / voff1); the descriptor base
  // walks through the channels by one scalar addition per step.  The steps arrive in order (0, 1, 2, ... and the last one
  // repeated at the tail: `act_s` is the step the base points at), so the switch from in0 to in1 is taken exactly once.
  auto load_act = [&](int s) {
    if (WINO_ABL(2)) return;
    if (s != act_s) {
      act_s = s;
      act_base += KC * HW * 4;
      if (s * KC == p.c0) {
        act_base = reinterpret_cast<uintptr_t>(p.in1) - 16;
#pragma unroll
        for (int i = 0; i < 4; ++i) voff[i] = voff1[i];
      }
    }
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(reinterpret_cast<const void*>(act_base), 0x7fffffff);
#pragma unroll
    for (int i = 0; i < 4; ++i) rb[i] = buf_load4(rx, voff[i], 0);
  };
  auto stage_act = [&](auto bufc) {  // rb -> ReLU-on-load, B^T d B -> sB(buf)
    const int buf = bufc;
    float* bdst = sB(buf) + (sh * 4 + sm) * 64 + st;  // position q at + q * 8 * 64
    f32x2 dl[4], dr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x4 v = rb[i];
      if (RELU) {
        dl[i] = f32x2{__builtin_amdgcn_fmed3f(v[0], 0.0f, llim), __builtin_amdgcn_fmed3f(v[1], 0.0f, pinf)};
        dr[i] = f32x2{__builtin_amdgcn_fmed3f(v[2], 0.0f, pinf), __builtin_amdgcn_fmed3f(v[3], 0.0f, rlim)};
      } else {
        dl[i] = f32x2{lcol ? v[0] : 0.0f, v[1]};
        dr[i] = f32x2{v[2], rcol ? v[3] : 0.0f};
      }
    }
    f32x2 wl[4], wr[4];
    wl[0] = pk_sub(dl[0], dl[2]);
    wl[1] = pk_add(dl[1], dl[2]);
    wl[2] = pk_sub(dl[2], dl[1]);
    wl[3] = pk_sub(dl[1], dl[3]);
    wr[0] = pk_sub(dr[0], dr[2]);
    wr[1] = pk_add(dr[1], dr[2]);
    wr[2] = pk_sub(dr[2], dr[1]);
    wr[3] = pk_sub(dr[1], dr[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x2 lo, hi;  // (w0 - w2, w1 + w2), (w2 - w1, w1 - w3) of the row (w0, w1 | w2, w3)
      asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(lo) : "v"(wl[i]), "v"(wr[i]));
      asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[1,0]" : "=v"(hi) : "v"(wr[i]), "v"(wl[i]));
      if (WINO_ABL(1)) {
        asm volatile("" ::"v"(lo), "v"(hi));
        continue;
      }
      bdst[(4 * i + 0) * 8 * 64] = lo[0];
      bdst[(4 * i + 1) * 8 * 64] = lo[1];
      bdst[(4 * i + 2) * 8 * 64] = hi[0];
      bdst[(4 * i + 3) * 8 * 64] = hi[1];
    }
  };

  // fragments of position 8 ph + j: A = 16 bytes (the four k values of the lane's channel and k parity), B = four floats
  f32x4 fa[2][2], fb[2][2];
  const float* a_rd0 = sA(0) + ((8 * ph) * 2 * 64 + half * 64 + wm * 32 + l31) * 4;
  const float* b_rd0 = sB(0) + ((8 * ph) * 2 + half) * 4 * 64 + wn * 32 + l31;
  auto read_frag = [&](auto bufc, int set, int g) {
    const int buf = bufc;
    const float* a_rd = a_rd0 + buf * TILE_FLOATS;
    const float* b_rd = b_rd0 + buf * TILE_FLOATS;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int q = 2 * g + j;
      fa[set][j] = *reinterpret_cast<const f32x4*>(a_rd + q * 2 * 64 * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) fb[set][j][e] = b_rd[(q * 2 * 4 + e) * 64];
    }
  };
  auto multiply = [&](int set, int g) {  // positions 2 g, 2 g + 1: consecutive MFMAs never share an accumulator
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[2 * g + j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][j][e], fb[set][j][e], acc[2 * g + j], 0, 0, 0);
  };
  // Workgroup barrier of the K loop: a raw s_barrier behind explicit waits (a __syncthreads() with a DMA outstanding drains
  // vmcnt(0)).  lgkmcnt(0): this wave's LDS stores of the next tile's activations.  vmcnt(4): its weight DMA of the tile
  // that is read behind the barrier -- the DMA is the OLDEST vector-memory operation in flight, and exactly the four
  // activation loads issued after it are younger; they stay in flight across the barrier.
  auto wg_barrier = [&]() {
    if (WINO_ABL(4)) return;
    __builtin_amdgcn_s_waitcnt(0x0074);  // vmcnt(4) lgkmcnt(0)
    asm volatile("s_barrier" ::: "memory");
  };
  constexpr std::integral_constant<int, 0> B0{};
  constexpr std::integral_constant<int, 1> B1{};

  // One K step on buffer `buf` (compile time: every LDS address of the step is a base register + immediate).  It runs
  // ACROSS the workgroup barrier: the fragments of its last two positions are in registers before the barrier, their MFMAs
  // are issued behind it and cover the LDS latency of the next step's first fragments.
  // Behind the barrier that ends step s, tile s + 2 goes into the buffers of tile s: the activations that were loaded a
  // step ago are transformed and stored, THEN the weight DMA is issued (with a DMA in flight the compiler waits vmcnt(0)
  // at the use of an ordinary load's result: here only those loads are outstanding), then the loads of tile s + 3 go out
  // (ONE register set: rb is free again).  Nothing in a step waits for a load younger than a step.
  // INVARIANT: the buffers of tile s are free behind that barrier ONLY because every wave has read its last fragments of
  // tile s (position pair 3, register set 1) BEFORE it; nothing reads sA(buf) / sB(buf) until tile s + 2 is complete (the
  // waits in front of the barrier that ends step s + 1).
  // Tile 1 has no barrier to go behind: every wave stages it in front of the barrier of step 0, as the previous form of
  // this kernel did for every tile (with ReLU-on-load behind the third MFMA group instead of the last: 2 % there).
  auto step = [&](auto bufc, int s) {
    const auto other = flip_buf(bufc);
    const bool tile1 = s == 0 && ksteps > 1;
    auto stage_tile1 = [&]() {
      stage_act(other);
      load_act(min(2, ksteps - 1));  // (always four loads behind a DMA: the barrier's counted wait)
    };
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      SCHED_PIN();
      read_frag(bufc, (g + 1) & 1, g + 1);
      SCHED_PIN();
      multiply(g & 1, g);
      SCHED_PIN();
      if (RELU && g == 2 && tile1) stage_tile1();
    }
    if (!RELU && tile1) stage_tile1();
    SCHED_PIN();
    wg_barrier();
    SCHED_PIN();
    if (s + 1 < ksteps) read_frag(other, 0, 0);
    SCHED_PIN();
    if (s + 2 < ksteps) {
      stage_act(bufc);
      load_w(s + 2, bufc);
      load_act(min(s + 3, ksteps - 1));
    }
    SCHED_PIN();
    multiply(1, 3);
    SCHED_PIN();
  };

  load_act(0);
  load_w(0, B0);
  stage_act(B0);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  read_frag(B0, 0, 0);
  if (ksteps > 1) {
    load_w(1, B1);
    load_act(1);
  }
  for (int s = 0;;) {  // unrolled by two with an exit after either half: odd counts and ksteps == 1 need no second body
    step(B0, s);
    if (++s == ksteps) break;
    step(B1, s);
    if (++s == ksteps) break;
  }
  // No DMA is in flight here (the last one, tile ksteps - 1, was waited for in front of the barrier of step ksteps - 2), but
  // the exchange area below is the weight tiles' space: the wait is unconditional
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- output stage, on all eight waves.  Rows of M held by this half -> partial t0 = (A^T M)[0], t1 = (A^T M)[1], then
  // the column pass:   ph = 0: t0 = M0 + M1, t1 = M1;      ph = 1: t0 = M2, t1 = -M2 - M3
  // Half ph finishes the accumulator rows 8 ph .. 8 ph + 7 (eight of the lane's sixteen output channels) and hands the
  // partials of the other eight over to the other half; (partial + partial) + bias + residual as before (the sum of the two
  // partials is commutative: bit-identical whichever half adds).
  float* xch = sA(0) + (wq * 16 * 4) * 64 + lane;  // [quadrant][r][a * 2 + j][lane]: 64 KB = both weight tiles
  const int n = n0 + wn * 32 + l31;
  const bool n_ok = n < p.n_tiles;
  int64_t o_base;
  int r_off;
  bool row1;  // the tile's second output row exists (odd heights: the last tile row has one)
  {
    const int nn = min(n, p.n_tiles - 1);
    const int b = nn / p.tiles_per_img;
    const int rr = nn - b * p.tiles_per_img;
    const int ty = rr / p.tiles_x, tx = rr - ty * p.tiles_x;
    const int64_t pix = (int64_t)(2 * ty) * p.W + 2 * tx;
    o_base = (int64_t)b * p.cout * HW + pix;
    r_off = (int)(((int64_t)b * p.res_bs + pix) * 4);
    row1 = 2 * ty + 1 < p.H;
  }
  const __amdgpu_buffer_rsrc_t rres = make_rsrc(RES ? p.res : p.out, RES ? 0x7fffffff : 0);
  auto partial = [&](auto phc, int r, float (&y)[2][2]) {
    if constexpr (decltype(phc)::value == 0) {
      const float a0 = acc[0][r] + acc[4][r], a1 = acc[1][r] + acc[5][r], a2 = acc[2][r] + acc[6][r], a3 = acc[3][r] + acc[7][r];
      y[0][0] = a0 + a1 + a2;
      y[0][1] = a1 - a2 - a3;
      const float b0 = acc[4][r], b1 = acc[5][r], b2 = acc[6][r], b3 = acc[7][r];
      y[1][0] = b0 + b1 + b2;
      y[1][1] = b1 - b2 - b3;
    } else {
      const float a0 = acc[0][r], a1 = acc[1][r], a2 = acc[2][r], a3 = acc[3][r];
      y[0][0] = a0 + a1 + a2;
      y[0][1] = a1 - a2 - a3;
      const float b0 = -acc[0][r] - acc[4][r], b1 = -acc[1][r] - acc[5][r], b2 = -acc[2][r] - acc[6][r], b3 = -acc[3][r] - acc[7][r];
      y[1][0] = b0 + b1 + b2;
      y[1][1] = b1 - b2 - b3;
    }
  };
  // residual and bias of the half's eight channels, fetched together and before any store (`out` may alias `res`)
  f32x2 rv[8][2];
  float bv[8];
  auto fetch = [&](auto phc) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int r = decltype(phc)::value * 8 + k;
      const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      bv[k] = p.bias ? p.bias[min(m, p.cout - 1)] : 0.0f;
      if (RES) {
        const int mo = (m < p.cout && n_ok) ? r_off + (int)((int64_t)m * HW * 4) : (int)0x80000000;
#pragma unroll
        for (int a = 0; a < 2; ++a)
          rv[k][a] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rres, (a == 0 || row1) ? mo + a * p.W * 4 : (int)0x80000000, 0, 0));
      } else {
        rv[k][0] = rv[k][1] = f32x2{0.0f, 0.0f};
      }
    }
  };
  auto hand_over = [&](auto phc) {  // the other half's rows
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int r = (1 - decltype(phc)::value) * 8 + k;
      float y[2][2];
      partial(phc, r, y);
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int j = 0; j < 2; ++j) xch[(r * 4 + a * 2 + j) * 64] = y[a][j];
    }
  };
  // (kept in scalar registers: read through `p` they are fetched again for every row, each fetch a wait)
  int act = p.act;
  float* outp = p.out;
  asm("" : "+s"(act), "+s"(outp));
  auto finish = [&](auto phc) {
    float xv[8][4];  // the other half's partials, all 32 reads in flight at once (read at the use, every one is a round trip)
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) xv[k][e] = xch[((decltype(phc)::value * 8 + k) * 4 + e) * 64];
    SCHED_PIN();
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int r = decltype(phc)::value * 8 + k;
      const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (m >= p.cout) continue;
      float y[2][2];
      partial(phc, r, y);
      const int64_t o = o_base + (int64_t)m * HW;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        f32x2 v;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          float x = (y[a][j] + xv[k][a * 2 + j]) + bv[k] + rv[k][a][j];
          if (act == DEVA_ACT_RELU) {
            x = fmaxf(x, 0.0f);
          } else if (act == DEVA_ACT_SIGMOID) {
            x = sigmoidf_(x);
          } else if (act == DEVA_ACT_SQUARE_PLUS_ONE) {
            x = x * x + 1.0f;
          }
          v[j] = x;
        }
        if (a == 0 || row1) *reinterpret_cast<f32x2*>(outp + o + (int64_t)a * p.W) = v;
      }
    }
  };
  if (ph == 0) {
    fetch(B0);
    SCHED_PIN();
    hand_over(B0);
  } else {
    fetch(B1);
    SCHED_PIN();
    hand_over(B1);
  }
  // (a raw barrier: the LDS stores are waited for, the residual / bias loads stay in flight across it)
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  asm volatile("s_barrier" ::: "memory");
  if (!n_ok) return;
  if (ph == 0) {
    finish(B0);
  } else {
    finish(B1);
  }
}

#undef sA
#undef sB
#undef SCHED_PIN

}  // namespace

static_assert(KC == kWinoKC && WM == kWinoBM && WN == kWinoBN, "what the planner assumes of this kernel");

int launch_conv_wino(const ConvArgs& a, const float* u, const deva_conv_launch& l, hipStream_t st) {
  WinoArgs p;
  p.in0 = a.in0;
  p.in1 = a.in1 ? a.in1 : a.in0;
  p.bs0 = a.bs0;
  p.bs1 = a.bs1;
  p.c0 = a.c0;
  p.ctot = a.ctot;
  p.H = a.H;
  p.W = a.W;
  p.tiles_x = a.W / 2;
  p.tiles_per_img = ((a.H + 1) / 2) * (a.W / 2);
  const int batch = a.n_total / a.OHW;
  p.n_tiles = batch * p.tiles_per_img;
  p.u = u;
  p.bias = a.bias;
  p.cout = a.cout;
  p.cout_pad = (a.cout + 63) / 64 * 64;
  p.relu_in = a.relu_in;
  p.res = a.res;
  p.res_bs = a.res_bs;
  p.act = a.act;
  p.out = a.out;
  p.blocks_m = p.cout_pad / WM;
  p.ablate = 0;
#ifdef DEVA_CONV_PROBES
  static const int ablate_probe = [] {
    const char* e = getenv("DEVA_WINO_ABLATE");
    return e ? atoi(e) : 0;
  }();
  p.ablate = ablate_probe;
#endif
  p.by_tiles = l.kind;
  if (p.blocks_m != l.tiles_m || (int64_t)l.tiles_m * l.tiles_n != l.grid_x) {
    set_error("deva_conv2d: the plan's Winograd grid (%d x %d) does not fit the kernel's %d cout blocks", l.tiles_m, l.tiles_n, p.blocks_m);
    return 2;
  }
  const dim3 grid(l.grid_x), block(l.block);
  if (p.relu_in) {
    if (p.res) {
      hipLaunchKernelGGL((conv_wino_kernel<true, true>), grid, block, 0, st, p);
    } else {
      hipLaunchKernelGGL((conv_wino_kernel<true, false>), grid, block, 0, st, p);
    }
  } else {
    if (p.res) {
      hipLaunchKernelGGL((conv_wino_kernel<false, true>), grid, block, 0, st, p);
    } else {
      hipLaunchKernelGGL((conv_wino_kernel<false, false>), grid, block, 0, st, p);
    }
  }
  return check_launch("deva_conv2d (Winograd F(2x2, 3x3))");
}

}  // namespace deva

// Host-side weight transform (model load): w_oihw [cout][cin][3][3] (BatchNorm folded), cin % 8 == 0 -> U = G g G^T in the
// layout the kernel stages: element (c, p = 4 i + l, m) at ((((c/8)*16 + p)*2 + c%2)*cout_pad64 + m)*4 + (c%8)/2, cout padded
// to a multiple of 64 with zeros; computed in fp64, rounded once.  Returns the number of floats (out == NULL: size query), -1 when
// the layer is not eligible.
extern "C" int64_t deva_conv_pack_wino(const float* w_oihw, float* out, int cout, int cin) {
  using namespace deva;
  if (!w_oihw || cout <= 0 || cin <= 0) {
    set_error("deva_conv_pack_wino: bad arguments");
    return -1;
  }
  if (cin % 8) return -1;
  const int cout_pad = (cout + 63) / 64 * 64;
  const int64_t elems = (int64_t)(cin / 8) * 16 * 2 * cout_pad * 4;
  if (!out) return elems;
  for (int64_t i = 0; i < elems; ++i) out[i] = 0.0f;
  static const double G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
  for (int m = 0; m < cout; ++m)
    for (int c = 0; c < cin; ++c) {
      const float* g = w_oihw + ((int64_t)m * cin + c) * 9;
      double t[4][3];
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 3; ++j) t[i][j] = G[i][0] * g[0 * 3 + j] + G[i][1] * g[1 * 3 + j] + G[i][2] * g[2 * 3 + j];
      for (int i = 0; i < 4; ++i)
        for (int l = 0; l < 4; ++l) {
          const double u = t[i][0] * G[l][0] + t[i][1] * G[l][1] + t[i][2] * G[l][2];
          const int q = 4 * i + l;
          out[((((int64_t)(c / 8) * 16 + q) * 2 + (c & 1)) * cout_pad + m) * 4 + (c % 8) / 2] = (float)u;
        }
    }
  return elems;
}
