// Stand-alone driver of the HIP-free host code of the low-resolution filter (csrc/lowres/lowres_plan.cpp: the checks of rule
// L7 of its three launching entry points and the launch decision) for tests/test_lowres_cpu.py, which builds it with
// -fsanitize=address,undefined.  It walks the checks over the product of their boundary values with made-up addresses
// (nothing is dereferenced), holds every accepted plan to its own promises -- the band, the grid, the LDS budget, the
// path rule -- and, with rule L1 evaluated here in fp32 as the kernels evaluate it, to the one promise the kernels rely
// on: no band touches more rows of `mid` or of `low` than the plan reserves.  It prints "checks refused failures".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "deva_lowres.h"
#include "lowres_plan.h"

using namespace deva_lowres;

static long checks = 0, refused = 0, failures = 0;

static void expect(bool ok, const char* what, const struct deva_lowres_geometry& g) {
  if (ok) return;
  ++failures;
  if (failures < 20)
    fprintf(stderr, "FAIL %s: low %d x %d, M %d, input %d x %d, out %d x %d\n", what, g.low_h, g.low_w, g.model_size, g.in_h, g.in_w,
            g.out_h, g.out_w);
}

static bool geometry_ok(const struct deva_lowres_geometry& g) {
  return g.low_h >= 1 && g.low_h <= 4096 && g.low_w >= 1 && g.low_w <= 4096 && g.model_size >= 1 && g.model_size <= 4096 && g.in_h >= 1 &&
         g.in_h <= g.model_size && g.in_w >= 1 && g.in_w <= g.model_size && g.out_h >= 1 && g.out_w >= 1 &&
         (int64_t)g.out_h * g.out_w <= (1ll << 30) && g.reserved == 0;
}

// L1, as lowres.hip's lowres_axis has it
static void axis(float scale, int d, int n_in, int* i0, int* i1) {
  float s = scale * ((float)d + 0.5f) - 0.5f;
  if (!(s > 0.0f)) s = 0.0f;
  *i0 = (int)s < n_in - 1 ? (int)s : n_in - 1;
  *i1 = *i0 + 1 < n_in - 1 ? *i0 + 1 : n_in - 1;
}

static void band_fits(const struct deva_lowres_geometry& g, const struct deva_lowres_plan& p, int band) {
  const float s2y = axis_scale(g.in_h, g.out_h), s1y = axis_scale(g.low_h, g.model_size);
  const int r0 = band * p.tile_rows;
  const int r_last = (r0 + p.cover_rows < g.out_h ? r0 + p.cover_rows : g.out_h) - 1;
  int my_lo, my_hi, ly_lo, ly_hi, unused;
  axis(s2y, r0, g.in_h, &my_lo, &unused);
  axis(s2y, r_last, g.in_h, &unused, &my_hi);
  expect(my_hi - my_lo + 1 <= p.mid_rows, "a band touches more rows of mid than the plan reserves", g);
  axis(s1y, my_lo, g.low_h, &ly_lo, &unused);
  axis(s1y, my_hi, g.low_h, &unused, &ly_hi);
  expect(ly_hi - ly_lo + 1 <= p.low_rows, "a band touches more rows of low than the plan reserves", g);
}

static void plan_holds(const struct deva_lowres_geometry& g, const struct deva_lowres_plan& p) {
  expect(p.path == DEVA_LOWRES_PATH_TILE || p.path == DEVA_LOWRES_PATH_POINT, "path", g);
  expect(p.tile_rows >= 1 && p.tile_rows <= DEVA_LOWRES_MAX_TILE_ROWS && p.tile_rows <= g.out_h, "tile_rows", g);
  expect(p.tile_cols == g.out_w && p.block == kBlock && p.grid_y_max == (uint32_t)kMaxGridY, "constants", g);
  expect((int64_t)p.grid_x * p.tile_rows >= g.out_h && ((int64_t)p.grid_x - 1) * p.tile_rows < g.out_h, "grid_x", g);
  expect(p.cover_rows >= p.tile_rows && p.cover_rows <= g.out_h, "cover_rows", g);
  // a piece of 16 pixels that starts in the last row of a band ends within cover_rows of the band's first row
  expect(p.cover_rows == g.out_h || (int64_t)(p.cover_rows - p.tile_rows) * g.out_w >= kPiece - 1, "reach", g);
  expect(p.out_values == (int64_t)p.tile_rows * g.out_w, "out_values", g);
  if (p.path == DEVA_LOWRES_PATH_POINT) {
    expect(p.lds_bytes == 0 && p.mid_rows == 0 && p.low_rows == 0 && p.mid_values == 4 * p.out_values, "point path", g);
    return;
  }
  expect(p.lds_bytes == 4 * (p.mid_rows * g.in_w + p.low_rows * g.low_w) && p.lds_bytes <= DEVA_LOWRES_LDS_BUDGET, "lds_bytes", g);
  expect(p.mid_rows >= 1 && p.mid_rows <= g.in_h && p.low_rows >= 1 && p.low_rows <= g.low_h, "patch rows", g);
  expect(p.mid_values == (int64_t)p.mid_rows * g.in_w && p.mid_values <= kMidPerOutMax * p.out_values, "mid_values", g);
  const int64_t bands = p.grid_x;
  for (int64_t b = 0; b < bands; b = b < 64 || b + 65 >= bands ? b + 1 : bands - 64) band_fits(g, p, (int)b);  // both ends
}

int main() {
  const void* ptr = reinterpret_cast<const void*>((uintptr_t)1 << 40);
  const void* odd = reinterpret_cast<const void*>(((uintptr_t)1 << 40) + 2);
  struct deva_lowres_plan plan;
  const int lows[] = {0, 1, 8, 16, 255, 256, 4096, 4097};
  const int models[] = {0, 1, 32, 64, 1024, 4096, 4097};
  const int outs[] = {0, 1, 2, 5, 9, 15, 16, 17, 33, 70, 129, 480, 854, 1080, 1920, 3840, 32768, 1 << 30, (1 << 30) + 1};
  for (int lh : lows)
    for (int lw : {1, 16, 256, 4097})
      for (int m : models)
        for (int ih : {0, 1, m / 2 + 1, (m * 9 + 15) / 16, m, m + 1})
          for (int iw : {1, m, m + 1})
            for (int oh : outs)
              for (int ow : outs) {
                struct deva_lowres_geometry g = {lh, lw, m, ih, iw, oh, ow, 0};
                memset(&plan, 0x5a, sizeof plan);
                const int rc = deva_lowres_plan(&g, &plan);
                ++checks;
                if (rc) ++refused;
                expect((rc == 0) == geometry_ok(g), "deva_lowres_plan accepts exactly the geometries of L7", g);
                expect(rc == 0 || (rc == 2 && deva_lowres_last_error()[0]), "a refusal is code 2 with a text", g);
                if (rc == 0) plan_holds(g, plan);
              }
  // the pointers, batches and thresholds of the three launching entry points, on a small and on a real geometry
  const double nan = __builtin_nan("");
  for (struct deva_lowres_geometry g : {deva_lowres_geometry{16, 16, 64, 36, 64, 33, 70, 0}, deva_lowres_geometry{256, 256, 1024, 576, 1024, 1080, 1920, 0},
                                        deva_lowres_geometry{16, 16, 64, 36, 64, 33, 70, 1}})
    for (int batch : {-1, 0, 1, 1100, 1 << 30})
      for (const void* low : {(const void*)nullptr, ptr, odd})
        for (const void* out : {(const void*)nullptr, ptr, odd}) {
          const bool geo = geometry_ok(g);
          int rc = upsample_check(low, batch, &g, out, &plan);
          ++checks, refused += rc != 0;
          expect((rc == 0) == (geo && batch >= 0 && (batch == 0 || (low == ptr && out == ptr))), "upsample_check", g);
          for (int per_box : {0, 1, 3, 16, 17})
            for (const void* scores : {(const void*)nullptr, ptr, odd})
              for (double t : {0.0, nan}) {
                rc = select_check(low, scores, batch, per_box, &g, t, out, nullptr, &plan);
                ++checks, refused += rc != 0;
                const bool sizes = geo && batch >= 0 && per_box >= 1 && per_box <= 16 && (int64_t)batch * per_box <= (1ll << 30) && t == t;
                const bool rest = batch == 0 || (low == ptr && out != nullptr && scores != odd && (scores || per_box == 1));
                expect((rc == 0) == (sizes && rest), "select_check", g);
              }
          for (int capacity : {0, 1, 4096, 4097})
            for (const void* scratch : {(const void*)nullptr, ptr, odd})
              for (int64_t bytes : {(int64_t)0, (int64_t)1 << 30})
                for (double t : {0.88, nan}) {
                  rc = proposal_check(low, out, batch, &g, t, 0.95, 1.0, 0.0, ptr, capacity, scratch, bytes, &plan);
                  ++checks, refused += rc != 0;
                  const bool sizes = geo && batch >= 0 && t == t && capacity >= 1 && capacity <= 4096 && scratch == ptr && bytes > 0;
                  expect((rc == 0) == (sizes && (batch == 0 || (low == ptr && out == ptr))), "proposal_check", g);
                }
        }
  struct deva_lowres_geometry g = {16, 16, 64, 36, 64, 33, 70, 0};
  ++checks, refused += deva_lowres_plan(nullptr, &plan) == 2;
  ++checks, refused += deva_lowres_plan(&g, nullptr) == 2;
  ++checks, refused += deva_lowres_limits(nullptr) == 2;
  expect(proposal_check(ptr, ptr, 1, &g, 0.88, 0.95, 1.0, 0.0, nullptr, 8, ptr, 1 << 30, &plan) == 2, "a null arena is refused", g);
  expect(deva_lowres_version() == DEVA_LOWRES_ABI_VERSION, "version", g);
  printf("%ld %ld %ld\n", checks, refused, failures);
  return failures ? 1 : 0;
}
