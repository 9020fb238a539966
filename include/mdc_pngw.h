/*
 * mdc_pngw.h -- C interface of libmdc_pngw.so: a PNG encoder for device-resident grayscale images, 8-bit and 16-bit.
 *
 * The output layout is the one mdcj_encode_*_device (include/mdc_jenc.h) leaves and mdcz_append_device (include/mdc_zipw.h)
 * archives: file f at d_out + f * slot_bytes (a 64-bit offset), its length in int32_t d_sizes[f].  A library of its own:
 * libmdc_hip.so / libmdc_host.so neither link nor load it, and it needs no mdc_ctx.  It links libmdc_zipw.so for one function,
 * mdcz_crc32_device, which gives the IDAT chunk's CRC.
 *
 * The file.  Signature; IHDR (width, height, depth 8 or 16, colour type 0, compression 0, filter 0, no interlace); exactly one
 * IDAT; IEND.  Nothing else, so the file is a pure function of the pixels and the options.  16-bit samples are uint16_t in host
 * order on the device and big-endian in the file.  IDAT holds a zlib stream: the header 78 01, one DEFLATE stream, the Adler-32
 * of the filtered bytes, big-endian.
 *
 * Filtering.  The filtered image is h rows of 1 + w * bpp bytes (bpp = depth / 8): the row's filter type, then its bytes.  The five
 * PNG filter types work on bytes, with a = the byte bpp to the left, b = the byte above, c = the byte above a (missing ones are
 * 0): 0 x; 1 x - a; 2 x - b; 3 x - ((a + b) >> 1); 4 x - paeth(a, b, c), all mod 256, computed from the RAW neighbours, so every
 * row is independent.  `filter` 0..4 forces one type for every row.  MDCP_FILTER_ADAPTIVE takes, per row, the type whose
 * filtered bytes (the type byte not counted) have the smallest sum taken as signed, sum |int8|; ties go to the lowest type
 * (libpng's heuristic).
 *
 * DEFLATE, Huffman only: no LZ77 matches (see the limits).  One dynamic block (BFINAL 1, BTYPE 2) per image.  The histogram of
 * the F = h * (1 + w * bpp) filtered bytes plus one end-of-block gives the literal/length code over 257 symbols (HLIT = 0),
 * limited to 15 bits.  HDIST = 0: one distance code, of length 0 ("no distance codes are used", RFC 1951 3.2.7).  The 258 code
 * lengths (257 + the distance code's 0) are run-length coded as ONE sequence, greedily from the left.  A run of r equal values v:
 *   v == 0: while r >= 11: symbol 18 with n = min(r, 138) (7 extra bits, n - 11), r -= n; then r >= 3: symbol 17 (3 extra bits,
 *           r - 3); else r literal zeros.
 *   v != 0: the value itself once, r -= 1; while r >= 3: symbol 16 with n = min(r, 6) (2 extra bits, n - 3), r -= n; then r times v.
 * The code-length code over these symbols is limited to 7 bits; HCLEN is the last used position of the order 16 17 18 0 8 7 9 6
 * 10 5 11 4 12 3 13 2 14 1 15, at least 4.  Codes are canonical (RFC 1951 3.2.2) and the bit stream is LSB-first.
 *
 * Code lengths (mdcp_huffman_lengths_device runs exactly this; counts are uint32_t, weights are summed in 64 bits):
 *   1. The used symbols (count > 0) in ascending order of (count, symbol): L[0..n).  n == 0: all lengths 0.  n == 1: length 1.
 *   2. Huffman's algorithm with two queues: the leaves in that order, and the internal nodes in the order they are made.  Each of
 *      the two nodes of a step is the front leaf if there is one and (no internal node is waiting or the leaf's weight <= the front
 *      internal node's weight), else the front internal node.  A symbol's length is its leaf's depth, cut to `limit`.
 *   3. With K = sum 2^(limit - length): while K > 2^limit, sweep L from the front (rarest first); every symbol with length <
 *      limit gets one bit longer (K -= 2^(limit - new length)), the sweep stopping as soon as K <= 2^limit.
 *   4. While K < 2^limit: the LAST symbol of L (the most frequent first) with 2^(limit - length) <= 2^limit - K gets one bit shorter
 *      (K += 2^(limit - old length)).  One always exists: the deficit is a multiple of the longest code's share.
 *   The result is within the limit and, for n >= 2, Kraft-complete.  It needs n <= 2^limit.
 *
 * Stored fallback, decided on the device per image: with D = the dynamic DEFLATE stream's bytes (header, codes, end-of-block,
 * padded to a byte) and S = F + 5 * ceil(F / 65535), the image is written as stored blocks of at most 65535 bytes (each 5 bytes:
 * BFINAL on the last, LEN, ~LEN) unless D < S.  So mdcp_png_bound(w, h, depth) = 57 + 6 + S is exact for the stored form and an
 * upper bound of every file: 57 = signature 8 + IHDR 25 + IDAT framing 12 + IEND 12, 6 = zlib header + Adler-32.
 *
 * Float input is converted as mdcj_encode_f32_device does: rintf (ties to even), clamped to 0..255, NaN -> 0.
 *
 * Limits, each checked and reported as an error status (never a fault):
 *   1 <= w, h; depth 8 or 16; filter 0..4 or MDCP_FILTER_ADAPTIVE; mdcp_png_bound(w, h, depth) <= 2^31 - 1 (sizes are int32_t, and
 *   every position inside an image fits 31 bits; bit offsets are 64-bit); 1 <= max_images; the scratch arrays, max_images *
 *   (24 * ceil(F / 16) + 2792) bytes (the filtered bytes, a 64-bit bit offset per 16 of them, tables), at most 2^40 bytes;
 *   per call 0 <= nimages <= max_images, stride >= w * h elements, slot_bytes >= the bound, 16-bit images 2-byte aligned, float
 *   images 4-byte aligned; d_out and slot_bytes of any alignment.  Offsets across the batch are 64-bit.
 *   No LZ77 in this library: a smooth image is coded at its zeroth-order entropy, not below -- unless it is encoded by
 *   libmdc_pnglz.so (include/mdc_pnglz.h), which writes the same file with matches where they make it smaller.  The code builder and the scan over an image's bit
 *   offsets run in one workgroup per image: the encoder is made for batches of images, not for one large image.
 *
 * Threads: an encoder holds the scratch arrays of one call at a time -- calls on one encoder are ordered by the caller (same
 * stream, or synchronised); different encoders are independent.  The encode calls enqueue on `stream` (hipStream_t as void*,
 * NULL = the default stream) and do not synchronise.
 */
#ifndef MDC_PNGW_H
#define MDC_PNGW_H
#include <stddef.h>
#include <stdint.h>
#ifndef MDC_API
#if defined(__GNUC__) || defined(__clang__)
#define MDC_API __attribute__((visibility("default")))
#else
#define MDC_API
#endif
#endif
#ifdef __cplusplus
extern "C" {
#endif

#define MDCP_OK 0
#define MDCP_ERR_ARG (-1)       /* null pointer, depth / filter / nimages / stride / alignment out of range */
#define MDCP_ERR_SIZE (-3)      /* w, h, the bound or the scratch beyond the limits above; slot_bytes below the bound */
#define MDCP_ERR_HIP (-4)       /* a HIP call failed */
#define MDCP_ERR_NO_DEVICE (-5) /* no such HIP device */
#define MDCP_ERR_NOMEM (-6)     /* the scratch arrays could not be allocated */

#define MDCP_FILTER_ADAPTIVE 5
#define MDCP_MAX_SYMBOLS 288 /* of mdcp_huffman_lengths_device */

typedef struct mdcp_encoder mdcp_encoder;

/* Exact size in bytes of a w x h image of `depth` bits written in the stored form, the upper bound of every file (derivation
 * above); -1 when w or h is below 1, depth is neither 8 nor 16, or the result passes 2^31 - 1. */
MDC_API int64_t mdcp_png_bound(int w, int h, int depth);

/* The message of the calling thread's last failed mdcp_* call ("" if none). */
MDC_API const char* mdcp_last_error(void);

/* An encoder for images of w x h at `depth` bits with `filter` on HIP device `device` (-1 = the calling thread's current
 * device), with scratch arrays for up to max_images images per call. */
MDC_API int mdcp_create(int device, int w, int h, int depth, int filter, int max_images, mdcp_encoder** out);
MDC_API void mdcp_destroy(mdcp_encoder* enc);

/* nimages images, image f = w * h elements (rows of w, no padding) at d_images + f * stride (in elements)  ->  its PNG file at
 * d_out + f * slot_bytes, and the file's length in d_sizes[f].  Nothing outside [f * slot_bytes, f * slot_bytes + d_sizes[f]) is
 * written.  u8 and f32 need an encoder of depth 8, u16 one of depth 16. */
MDC_API int mdcp_encode_u8_device(mdcp_encoder* enc, const uint8_t* d_images, int64_t stride, int nimages, uint8_t* d_out, int64_t slot_bytes,
                                  int32_t* d_sizes, void* stream);
MDC_API int mdcp_encode_u16_device(mdcp_encoder* enc, const uint16_t* d_images, int64_t stride, int nimages, uint8_t* d_out, int64_t slot_bytes,
                                   int32_t* d_sizes, void* stream);
/* The file of mdcp_encode_u8_device on the converted values. */
MDC_API int mdcp_encode_f32_device(mdcp_encoder* enc, const float* d_images, int64_t stride, int nimages, uint8_t* d_out, int64_t slot_bytes,
                                   int32_t* d_sizes, void* stream);

/* Output arrays owned by the encoder, for callers without an allocator of their own: max_images slots of *slot_bytes =
 * mdcp_png_bound(w, h, depth) and max_images sizes, allocated on the first call and freed by mdcp_destroy. */
MDC_API int mdcp_output_device(mdcp_encoder* enc, uint8_t** d_out, int64_t* slot_bytes, int32_t** d_sizes);

/* For tests: d_lengths[s] = the code length of symbol s for the counts d_hist[0 .. nsym), by the rule above, in one workgroup.
 * 1 <= nsym <= MDCP_MAX_SYMBOLS, 1 <= limit <= 15, nsym <= 2^limit. */
MDC_API int mdcp_huffman_lengths_device(const uint32_t* d_hist, int nsym, int limit, uint8_t* d_lengths, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDC_PNGW_H */
