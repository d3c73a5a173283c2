/* C ABI of libdeva_rle_text.so: the text of COCO run-length masks (the COCO API's rleToString / rleFrString) coded and
 * parsed on the device: run boundaries -> compressed strings, and compressed strings -> the run array of deva_rle.h (a
 * ninth library next to libdeva_hip.so, libdeva_metrics.so, libdeva_vos_metrics.so, libdeva_pair_metrics.so,
 * libdeva_regions.so, libdeva_rle.so, libdeva_mask_runs.so and libdeva_rle_overlap.so).  Every entry point is prefixed
 * deva_text_ and no symbol is defined in any two of the nine libraries.
 *
 * All functions that return int return 0 on success and non-zero on failure; the text of the last failure of the
 * calling thread is behind deva_text_last_error().  Every argument check is made before any launch.  Nothing is
 * allocated and nothing is synchronised: inputs, scratch and outputs are the caller's, and every kernel goes to the
 * stream that is handed in.
 *
 * Rules.  tests/rle_text_case.py is their executable statement.
 *   C1  a value.  A signed integer x is written low 5 bits first, one character per 5 bits: c = x & 0x1f; x >>= 5
 *       (arithmetic shift); more = (c & 0x10) ? x != -1 : x != 0; the character is (c | more << 5) + 48.  Reading is the
 *       inverse: characters are '0'..'o' (48..111), bit 0x20 of char - 48 announces another character, and if the last
 *       character of a value has bit 0x10 the bits above 5 * width are filled with ones.
 *   C2  the chain.  The counts c_0, c_1, c_2 of a mask are coded as they are, every later c_j as c_j - c_{j-2}.
 *   C3  encoder input: what deva_runs_count / deva_runs_write (or deva_mask_rle_count / _write) leave on the device.
 *       n int32 [N], base int64 [N], bounds int32 [bounds_len]; total = H * W with 1 <= H * W < 2^31.  The counts of
 *       mask k are diff([0, *bounds[base[k] .. base[k] + n[k]), H * W]), so a mask has n[k] + 1 counts: a leading 0 for
 *       a mask that starts with a 1, the single count H * W for an empty mask.  The planes are never read.  A boundary
 *       whose slot is outside [0, bounds_len) is not read and counts as H * W (the caller's capacity was too small and
 *       it knows that from the encoder's `total`; the text of such a mask is unspecified).
 *   C4  encoder output.  chars uint8 [capacity] with the texts back to back in mask order, text_len int32 [N],
 *       text_base int64 [N], text_total int64 [1], all on the device.  text_base[k] = first + text_len[0] + ... +
 *       text_len[k-1] (`first`: an int64 on the device, the text_total of the call before when several calls fill one
 *       `chars`; NULL means 0).  A character whose slot is at or beyond `capacity` is not written, nothing is ever
 *       written at or beyond `capacity`, and text_total always holds the full sum: rule E5 of deva_mask_runs.h.  The
 *       coding is the canonical one of C1 (a value ends at the first character where it may).
 *       deva_text_max_chars(total) is the widest a value can be for this H * W: 5 at 1080p, 7 at most.
 *   C5  parser input.  chars uint8 [L] on the device, the texts of N masks back to back; text_first int64 [N + 1] on
 *       the device, ascending from 0 to L (a value outside [0, L] is clamped into it); H and W.  Non-canonical codings
 *       are legal, up to DEVA_TEXT_MAX_CHARS (12) characters a value.  Zero counts are legal anywhere.
 *   C6  parser output: the run array of include/deva_rle.h, exactly: first[0 .. N], then per mask s_0 = 0, s_1, ..., s_r,
 *       in the caller's int32 buffer of words_cap >= 2 N + 1 + L words (a mask cannot have more values than
 *       characters, so the buffer is sized without a synchronisation).  info int64 [2] on the device: info[0] the
 *       flag bits of C7, info[1] the words used.
 *   C7  flags.  DEVA_TEXT_FLAG_CHAR: a character outside '0'..'o'; _OPEN: a text that ends inside a value; _LONG: a
 *       value of more than 12 characters; _COUNT: a count below 0 or above H * W; _SUM: a mask whose counts do not sum
 *       to H * W (an empty text is such a mask).  The chain and the sums are computed in 64 bits.  With a flag set the
 *       contents of the run array are unspecified; but for any input bytes at all no kernel writes outside words_cap
 *       words, info and its own scratch: where things are stored depends on indices only, never on decoded values.
 *   C8  limits.  N and words_cap within what deva_text_limits reports (the limits of deva_rle.h: 65 536 masks, 2^26
 *       words); L < 2^31.  A violation is an error that names the argument; nothing is launched and the outputs stay
 *       untouched.
 *
 * The kernels.  Both directions give a workgroup of 256 lanes one mask and walk it DEVA_TEXT_SCAN_CHUNK items at a
 * time, four consecutive items a lane, with the carries in registers.
 *   encode  text_len   a lane takes four consecutive counts: it reads the seven boundaries they need, forms the values
 *                      (C2) and their widths (C1); the widths are summed over the workgroup and the steps.
 *           text_base  one workgroup turns text_len into text_base and text_total, DEVA_TEXT_MASK_CHUNK masks a step.
 *           write      the same walk again; an exclusive scan of the widths over the workgroup plus the carry of the
 *                      steps before gives every value its place, and its characters leave as byte stores under C4.
 *   parse   values     one lane per character: the characters that end a value are counted per mask and the flags CHAR
 *                      and OPEN are taken (into the scratch).
 *           first      one workgroup turns the value counts into first[0 .. N], writes info[1] and the flags so far.
 *           starts     one lane per character again.  A lane whose character ends a value reads the value back to
 *                      front (at most 11 characters before its own, never below the text's first character, so a value
 *                      that began in the stretch of the step before is read whole).  Three scans over the workgroup
 *                      follow, each with its carry: the rank of the value, the two interleaved sums of C2 (even and odd
 *                      counts, restarted at count 2), and the sum of the counts, which is the start s_{j+1}.
 * No kernel waits on another workgroup.  A single mask is one workgroup's work: many masks fill the device, one does not.
 */
#ifndef DEVA_RLE_TEXT_H
#define DEVA_RLE_TEXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEVA_TEXT_ABI_VERSION 1

#define DEVA_TEXT_MAX_MASKS 65536
#define DEVA_TEXT_MAX_WORDS 67108864 /* of the run array of one call: 2^26 words */
#define DEVA_TEXT_MAX_CHARS 12       /* characters of one coded value: 60 bits */
#define DEVA_TEXT_SCAN_CHUNK 1024    /* counts (encode) or characters (parse) of one step of the per-mask walk */
#define DEVA_TEXT_MASK_CHUNK 256     /* masks of one step of the cross-mask scan */

#define DEVA_TEXT_FLAG_CHAR 1
#define DEVA_TEXT_FLAG_OPEN 2
#define DEVA_TEXT_FLAG_LONG 4
#define DEVA_TEXT_FLAG_COUNT 8
#define DEVA_TEXT_FLAG_SUM 16

int deva_text_version(void);
const char* deva_text_last_error(void);

/* (struct tags only: the functions have the same names, so say `struct deva_text_limits`, `struct deva_text_plan`) */
struct deva_text_limits {
  int32_t max_masks;   /* masks of one call */
  int32_t max_words;   /* words_cap of one parse */
  int32_t max_chars;   /* DEVA_TEXT_MAX_CHARS */
  int32_t block;       /* lanes of a workgroup */
  int32_t scan_chunk;  /* DEVA_TEXT_SCAN_CHUNK */
  int32_t mask_chunk;  /* DEVA_TEXT_MASK_CHUNK */
};
int deva_text_limits(struct deva_text_limits* limits);

struct deva_text_plan {
  uint32_t mask_grid;           /* workgroups of every per-mask kernel: n */
  uint32_t scan_grid;           /* workgroups of the cross-mask scans: 1 (0 when n is 0) */
  int32_t mask_chunks;          /* steps of the cross-mask scan: ceil(n / mask_chunk) */
  int32_t items;                /* items a lane takes in one step: scan_chunk / block */
  int32_t value_chars;          /* deva_text_max_chars(height * width) */
  int32_t reserved;
  int64_t min_words;            /* the smallest words_cap a parse of n masks and `chars` characters takes: 2 n + 1 + chars */
  int64_t parse_scratch_bytes;  /* what deva_text_parse_scratch gives: 8 n */
};
/* the launch decision of both directions for n masks of height x width and `chars` characters of text (0 when only
 * the encoder is meant), host only: no device is touched, nothing is dereferenced but `plan` */
int deva_text_plan(int n, int height, int width, int64_t chars, struct deva_text_plan* plan);

/* the widest a coded value can be when every count is within [0, total]: host only; -1 unless 1 <= total < 2^31 */
int deva_text_max_chars(int64_t total);

/* bytes of the parser's scratch for n masks (4-byte aligned); -1 beyond the limits */
int64_t deva_text_parse_scratch(int n);

/* n_in int32 [n], base int64 [n], bounds int32 [bounds_len] (may be NULL when bounds_len is 0), on the device (C3);
 * text_len int32 [n], text_base int64 [n], text_total int64 [1] on the device; first: int64 [1] on the device or NULL
 * (C4).  n == 0 is a no-op that returns 0. */
int deva_text_encode_count(const int32_t* n_in, const int64_t* base, const int32_t* bounds, int64_t bounds_len, int n, int height,
                           int width, int32_t* text_len, int64_t* text_base, int64_t* text_total, const int64_t* first, void* stream);

/* after deva_text_encode_count of the same inputs on the same stream, with its text_base untouched: chars uint8
 * [capacity] on the device (may be NULL when capacity is 0).  n == 0 is a no-op that returns 0. */
int deva_text_encode_write(const int32_t* n_in, const int64_t* base, const int32_t* bounds, int64_t bounds_len, int n, int height,
                           int width, const int64_t* text_base, uint8_t* chars, int64_t capacity, void* stream);

/* chars uint8 [chars_len] (may be NULL when chars_len is 0), text_first int64 [n + 1], on the device (C5); scratch:
 * deva_text_parse_scratch(n) bytes on the device, 4-byte aligned; runs int32 [words_cap], info int64 [2] on the device
 * (C6, C7).  n == 0 writes first[0] = 0 and info = {0, 1}. */
int deva_text_parse(const uint8_t* chars, int64_t chars_len, const int64_t* text_first, int n, int height, int width, void* scratch,
                    int64_t scratch_bytes, int32_t* runs, int64_t words_cap, int64_t* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif
