// The argument checks, rule C8 and the launch decision of the run-length text codec (see rle_text_plan.h), and the
// library's host-only entry points.
#include "rle_text_plan.h"

namespace deva_text {

HOST_ARGS_DEFINE_ERROR_TEXT()
const char* last_error() { return g_err; }

int text_plan(const char* what, int n, int height, int width, int64_t chars, struct deva_text_plan* plan) {
  DEVA_TEXT_REQUIRE(plan, "%s: null plan", what);
  DEVA_TEXT_REQUIRE(height > 0 && width > 0 && (int64_t)height * width <= kMaxPixels, "%s: bad height x width %d x %d (1 <= H * W < 2^31)",
                    what, height, width);
  DEVA_TEXT_REQUIRE(n >= 0 && n <= DEVA_TEXT_MAX_MASKS, "%s: n: 0 to %d masks a call (got %d)", what, DEVA_TEXT_MAX_MASKS, n);
  DEVA_TEXT_REQUIRE(chars >= 0 && chars <= kMaxText, "%s: chars_len: 0 to 2^31 - 1 characters a call (got %lld)", what, (long long)chars);
  const int64_t min_words = 2ll * n + 1 + chars;
  DEVA_TEXT_REQUIRE(min_words <= DEVA_TEXT_MAX_WORDS, "%s: chars_len: %d masks and %lld characters need %lld words, a call takes %d", what, n,
                    (long long)chars, (long long)min_words, DEVA_TEXT_MAX_WORDS);
  plan->mask_grid = (uint32_t)n;
  plan->scan_grid = n > 0 ? 1u : 0u;
  plan->mask_chunks = (n + DEVA_TEXT_MASK_CHUNK - 1) / DEVA_TEXT_MASK_CHUNK;
  plan->items = kItems;
  plan->value_chars = deva_text_max_chars((int64_t)height * width);
  plan->reserved = 0;
  plan->min_words = min_words;
  plan->parse_scratch_bytes = (int64_t)n * kMaskScratchBytes;
  return 0;
}

// what both halves of the encoder read
static int input_check(const char* what, const int32_t* n_in, const int64_t* base, const int32_t* bounds, int64_t bounds_len, int n) {
  DEVA_TEXT_REQUIRE(bounds_len >= 0 && bounds_len <= (1ll << 60), "%s: bounds_len: 0 to 2^60 (got %lld)", what, (long long)bounds_len);
  if (n == 0) return 0;
  DEVA_TEXT_REQUIRE(n_in && aligned(n_in, 4), "%s: n_in: null or misaligned", what);
  DEVA_TEXT_REQUIRE(base && aligned(base, 8), "%s: base: null or misaligned", what);
  DEVA_TEXT_REQUIRE((bounds || bounds_len == 0) && aligned(bounds, 4), "%s: bounds: null or misaligned", what);
  return 0;
}

int count_check(const int32_t* n_in, const int64_t* base, const int32_t* bounds, int64_t bounds_len, int n, int height, int width,
                const int32_t* text_len, const int64_t* text_base, const int64_t* text_total, const int64_t* first,
                struct deva_text_plan* plan) {
  const char* what = "deva_text_encode_count";
  struct deva_text_plan local;
  if (!plan) plan = &local;
  if (int rc = text_plan(what, n, height, width, 0, plan)) return rc;
  if (int rc = input_check(what, n_in, base, bounds, bounds_len, n)) return rc;
  if (n == 0) return 0;
  DEVA_TEXT_REQUIRE(text_len && aligned(text_len, 4), "%s: text_len: null or misaligned", what);
  DEVA_TEXT_REQUIRE(text_base && aligned(text_base, 8), "%s: text_base: null or misaligned", what);
  DEVA_TEXT_REQUIRE(text_total && aligned(text_total, 8), "%s: text_total: null or misaligned", what);
  DEVA_TEXT_REQUIRE(aligned(first, 8), "%s: first: misaligned", what);
  DEVA_TEXT_REQUIRE(first != text_total, "%s: first: it must not be `text_total` itself", what);
  const struct { const char* name; const void* p; int64_t bytes; } ins[] = {
      {"n_in", n_in, 4ll * n}, {"base", base, 8ll * n}, {"bounds", bounds, 4 * bounds_len}, {"first", first, 8}};
  const struct { const char* name; const void* p; int64_t bytes; } outs[] = {
      {"text_len", text_len, 4ll * n}, {"text_base", text_base, 8ll * n}, {"text_total", text_total, 8}};
  for (const auto& o : outs) {
    for (const auto& i : ins) DEVA_TEXT_REQUIRE(!overlaps(o.p, o.bytes, i.p, i.bytes), "%s: %s overlaps %s", what, o.name, i.name);
    for (const auto& q : outs)
      DEVA_TEXT_REQUIRE(&o == &q || !overlaps(o.p, o.bytes, q.p, q.bytes), "%s: %s overlaps %s", what, o.name, q.name);
  }
  return 0;
}

int write_check(const int32_t* n_in, const int64_t* base, const int32_t* bounds, int64_t bounds_len, int n, int height, int width,
                const int64_t* text_base, const uint8_t* chars, int64_t capacity, struct deva_text_plan* plan) {
  const char* what = "deva_text_encode_write";
  struct deva_text_plan local;
  if (!plan) plan = &local;
  if (int rc = text_plan(what, n, height, width, 0, plan)) return rc;
  DEVA_TEXT_REQUIRE(capacity >= 0 && capacity <= (1ll << 60), "%s: capacity: 0 to 2^60 (got %lld)", what, (long long)capacity);
  if (int rc = input_check(what, n_in, base, bounds, bounds_len, n)) return rc;
  if (n == 0) return 0;
  DEVA_TEXT_REQUIRE(text_base && aligned(text_base, 8), "%s: text_base: null or misaligned", what);
  DEVA_TEXT_REQUIRE(chars || capacity == 0, "%s: chars: null", what);
  const struct { const char* name; const void* p; int64_t bytes; } ins[] = {
      {"n_in", n_in, 4ll * n}, {"base", base, 8ll * n}, {"bounds", bounds, 4 * bounds_len}, {"text_base", text_base, 8ll * n}};
  for (const auto& i : ins) DEVA_TEXT_REQUIRE(!overlaps(chars, capacity, i.p, i.bytes), "%s: chars overlaps %s", what, i.name);
  return 0;
}

int parse_check(const uint8_t* chars, int64_t chars_len, const int64_t* text_first, int n, int height, int width, const void* scratch,
                int64_t scratch_bytes, const int32_t* runs, int64_t words_cap, const int64_t* info, struct deva_text_plan* plan) {
  const char* what = "deva_text_parse";
  struct deva_text_plan local;
  if (!plan) plan = &local;
  if (int rc = text_plan(what, n, height, width, chars_len, plan)) return rc;
  DEVA_TEXT_REQUIRE(words_cap >= plan->min_words && words_cap <= DEVA_TEXT_MAX_WORDS,
                    "%s: words_cap: %lld given, %d masks and %lld characters need %lld (2 n + 1 + chars_len) and a call takes %d", what,
                    (long long)words_cap, n, (long long)chars_len, (long long)plan->min_words, DEVA_TEXT_MAX_WORDS);
  DEVA_TEXT_REQUIRE(chars || chars_len == 0, "%s: chars: null", what);
  DEVA_TEXT_REQUIRE(text_first && aligned(text_first, 8), "%s: text_first: null or misaligned", what);
  DEVA_TEXT_REQUIRE(n == 0 || (scratch && aligned(scratch, 4)), "%s: scratch: null or not 4-byte aligned", what);
  DEVA_TEXT_REQUIRE(scratch_bytes >= plan->parse_scratch_bytes, "%s: scratch_bytes: %lld given, deva_text_parse_scratch asks for %lld", what,
                    (long long)scratch_bytes, (long long)plan->parse_scratch_bytes);
  DEVA_TEXT_REQUIRE(runs && aligned(runs, 4), "%s: runs: null or misaligned", what);
  DEVA_TEXT_REQUIRE(info && aligned(info, 8), "%s: info: null or misaligned", what);
  const struct { const char* name; const void* p; int64_t bytes; } ins[] = {{"chars", chars, chars_len}, {"text_first", text_first, 8ll * (n + 1)}};
  const struct { const char* name; const void* p; int64_t bytes; } outs[] = {
      {"scratch", scratch, plan->parse_scratch_bytes}, {"runs", runs, 4 * words_cap}, {"info", info, 16}};
  for (const auto& o : outs) {
    for (const auto& i : ins) DEVA_TEXT_REQUIRE(!overlaps(o.p, o.bytes, i.p, i.bytes), "%s: %s overlaps %s", what, o.name, i.name);
    for (const auto& q : outs)
      DEVA_TEXT_REQUIRE(&o == &q || !overlaps(o.p, o.bytes, q.p, q.bytes), "%s: %s overlaps %s", what, o.name, q.name);
  }
  return 0;
}

}  // namespace deva_text

extern "C" int deva_text_version(void) { return DEVA_TEXT_ABI_VERSION; }
extern "C" const char* deva_text_last_error(void) { return deva_text::last_error(); }
extern "C" int deva_text_limits(struct deva_text_limits* limits) {
  DEVA_TEXT_REQUIRE(limits, "deva_text_limits: null limits");
  limits->max_masks = DEVA_TEXT_MAX_MASKS;
  limits->max_words = DEVA_TEXT_MAX_WORDS;
  limits->max_chars = DEVA_TEXT_MAX_CHARS;
  limits->block = deva_text::kBlock;
  limits->scan_chunk = DEVA_TEXT_SCAN_CHUNK;
  limits->mask_chunk = DEVA_TEXT_MASK_CHUNK;
  return 0;
}
extern "C" int deva_text_plan(int n, int height, int width, int64_t chars, struct deva_text_plan* plan) {
  return deva_text::text_plan("deva_text_plan", n, height, width, chars, plan);
}
extern "C" int deva_text_max_chars(int64_t total) {
  if (total < 1 || total > deva_text::kMaxPixels) return -1;
  const int plus = deva_text::value_chars(total), minus = deva_text::value_chars(-total);
  return plus > minus ? plus : minus;
}
extern "C" int64_t deva_text_parse_scratch(int n) {
  return n < 0 || n > DEVA_TEXT_MAX_MASKS ? -1 : (int64_t)n * deva_text::kMaskScratchBytes;
}
