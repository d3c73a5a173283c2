// The argument checks, the MCU and interval geometry and the sizes of the JPEG coder (see jpeg_plan.h), and the library's
// host-only entry points.
#include "jpeg_plan.h"

namespace deva_jpeg {

HOST_ARGS_DEFINE_ERROR_TEXT()
const char* last_error() { return g_err; }

int jpeg_plan(const char* what, int height, int width, int subsampling, int restart, struct deva_jpeg_plan* plan) {
  DEVA_JPEG_REQUIRE(plan, "%s: null plan", what);
  DEVA_JPEG_REQUIRE(subsampling == DEVA_JPEG_420 || subsampling == DEVA_JPEG_444, "%s: subsampling: 420 ('4:2:0') or 444 ('4:4:4') (got %d)", what,
                    subsampling);
  DEVA_JPEG_REQUIRE(height >= 1 && width >= 1 && height <= DEVA_JPEG_MAX_SIDE && width <= DEVA_JPEG_MAX_SIDE,
                    "%s: bad height x width %d x %d (1 to %d each)", what, height, width, DEVA_JPEG_MAX_SIDE);
  DEVA_JPEG_REQUIRE((int64_t)height * width * 3 <= DEVA_JPEG_MAX_BYTES, "%s: a plane of %d x %d x 3 bytes, a call takes %d", what, height, width,
                    DEVA_JPEG_MAX_BYTES);
  DEVA_JPEG_REQUIRE(restart >= 0 && restart <= DEVA_JPEG_MAX_RESTART, "%s: restart: 0 (one MCU row) to %d MCUs (got %d)", what, DEVA_JPEG_MAX_RESTART,
                    restart);
  const int mcu = subsampling == DEVA_JPEG_420 ? 16 : 8, per = subsampling == DEVA_JPEG_420 ? 6 : 3;
  plan->mcu = mcu;
  plan->mcus_x = (width + mcu - 1) / mcu;
  plan->mcus_y = (height + mcu - 1) / mcu;
  plan->blocks_per_mcu = per;
  plan->restart = restart ? restart : plan->mcus_x;          // (at most 2048 MCUs across: within the DRI field)
  const int64_t mcus = (int64_t)plan->mcus_x * plan->mcus_y;  // (at most 2^29 / 3 / 64 with the padding of one MCU each way: int32)
  plan->intervals = (int32_t)((mcus + plan->restart - 1) / plan->restart);
  plan->blocks = (int32_t)(mcus * per);
  plan->block = kBlock;
  plan->coef_bytes = 128ll * plan->blocks;
  const int64_t full = mcus < plan->restart ? mcus : plan->restart, last = mcus - (int64_t)(plan->intervals - 1) * plan->restart;
  plan->slot_bytes = (interval_worst(full * per) + 15) / 16 * 16 + 16;
  int64_t at[4];
  plan->scratch_bytes = scratch_layout(*plan, at);
  plan->worst_case = (plan->intervals - 1) * interval_worst((int64_t)plan->restart * per) + interval_worst(last * per) - 2;
  return 0;
}

int place_check(const char* what, int height, int width, int subsampling, int restart, const void* scratch, int64_t scratch_bytes,
                const uint8_t* out, int64_t capacity, const int64_t* info, struct deva_jpeg_plan* plan) {
  struct deva_jpeg_plan local;
  if (!plan) plan = &local;
  if (int rc = jpeg_plan(what, height, width, subsampling, restart, plan)) return rc;
  DEVA_JPEG_REQUIRE(capacity >= 0 && capacity <= (1ll << 40), "%s: capacity: 0 to 2^40 (got %lld)", what, (long long)capacity);
  DEVA_JPEG_REQUIRE(out || capacity == 0, "%s: out: null", what);
  DEVA_JPEG_REQUIRE(scratch && aligned(scratch, 16), "%s: scratch: null or not 16-byte aligned", what);
  DEVA_JPEG_REQUIRE(scratch_bytes >= plan->scratch_bytes, "%s: scratch_bytes: %lld given, deva_jpeg_plan asks for %lld", what,
                    (long long)scratch_bytes, (long long)plan->scratch_bytes);
  DEVA_JPEG_REQUIRE(info && aligned(info, 8), "%s: info: null or misaligned", what);
  DEVA_JPEG_REQUIRE(!overlaps(out, capacity, scratch, plan->scratch_bytes), "%s: out overlaps scratch", what);
  DEVA_JPEG_REQUIRE(!overlaps(info, 32, scratch, plan->scratch_bytes), "%s: info overlaps scratch", what);
  DEVA_JPEG_REQUIRE(!overlaps(info, 32, out, capacity), "%s: info overlaps out", what);
  return 0;
}

int scan_check(const uint8_t* plane, int height, int width, int quality, int subsampling, int restart, const void* scratch,
               int64_t scratch_bytes, const uint8_t* out, int64_t capacity, const int64_t* info, struct deva_jpeg_plan* plan) {
  const char* what = "deva_jpeg_scan";
  struct deva_jpeg_plan local;
  if (!plan) plan = &local;
  if (int rc = place_check(what, height, width, subsampling, restart, scratch, scratch_bytes, out, capacity, info, plan)) return rc;
  DEVA_JPEG_REQUIRE(quality >= 1 && quality <= 100, "%s: quality: 1 to 100 (got %d)", what, quality);
  DEVA_JPEG_REQUIRE(plane, "%s: plane: null", what);
  const int64_t bytes = (int64_t)height * width * 3;
  DEVA_JPEG_REQUIRE(!overlaps(plane, bytes, scratch, plan->scratch_bytes), "%s: plane overlaps scratch", what);
  DEVA_JPEG_REQUIRE(!overlaps(plane, bytes, out, capacity), "%s: plane overlaps out", what);
  DEVA_JPEG_REQUIRE(!overlaps(plane, bytes, info, 32), "%s: plane overlaps info", what);
  return 0;
}

}  // namespace deva_jpeg

extern "C" int deva_jpeg_version(void) { return DEVA_JPEG_ABI_VERSION; }
extern "C" const char* deva_jpeg_last_error(void) { return deva_jpeg::last_error(); }
extern "C" int deva_jpeg_limits(struct deva_jpeg_limits* limits) {
  DEVA_JPEG_REQUIRE(limits, "deva_jpeg_limits: null limits");
  limits->max_side = DEVA_JPEG_MAX_SIDE;
  limits->max_bytes = DEVA_JPEG_MAX_BYTES;
  limits->max_restart = DEVA_JPEG_MAX_RESTART;
  limits->block_bits = deva_jpeg::kBlockBits;
  limits->block = deva_jpeg::kBlock;
  limits->lds_bytes = deva_jpeg::kLdsBytes;
  return 0;
}
extern "C" int deva_jpeg_plan(int height, int width, int subsampling, int restart, struct deva_jpeg_plan* plan) {
  return deva_jpeg::jpeg_plan("deva_jpeg_plan", height, width, subsampling, restart, plan);
}
extern "C" int deva_jpeg_quant(int quality, uint8_t* tables) {
  DEVA_JPEG_REQUIRE(tables, "deva_jpeg_quant: null tables");
  DEVA_JPEG_REQUIRE(quality >= 1 && quality <= 100, "deva_jpeg_quant: quality: 1 to 100 (got %d)", quality);
  const deva_jpeg::QuantTables t = deva_jpeg::quant_tables(quality);
  for (int z = 0; z < 64; ++z) tables[z] = t.q[0][deva_jpeg::kZigzag[z]], tables[64 + z] = t.q[1][deva_jpeg::kZigzag[z]];
  return 0;
}
