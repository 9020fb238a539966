/*
 * mdc_pnglz.h -- C interface of libmdc_pnglz.so: the PNG encoder of include/mdc_pngw.h and include/mdc_pngw_rgb.h with LZ77 matches
 * in its DEFLATE stream, for device-resident images of three kinds: 8-bit gray, 16-bit gray, 8-bit RGB.
 *
 * A library of its own: libmdc_pngw.so and libmdc_pngw_rgb.so are not touched by it, nothing links it but bin/rectifyDataset, and it
 * links libmdc_zipw.so for one function, mdcz_crc32_device (the IDAT chunk's CRC).  The output layout is theirs: file f at d_out +
 * f * slot_bytes (a 64-bit offset), its length in int32_t d_sizes[f].
 *
 * The file is the one include/mdc_pngw.h describes (RGB: include/mdc_pngw_rgb.h): signature, IHDR, exactly one IDAT, IEND; the zlib
 * header 78 01 and the Adler-32 of the filtered bytes; the filtered image of h rows of 1 + w * bpp bytes (bpp = 1, 2, 3 for gray8,
 * gray16, rgb8: the filter distance), the five filter types and the adaptive rule; the bound mdcl_png_bound(w, h, kind) =
 * mdcp_png_bound(w, h, 8 or 16) or mdcp_png_bound_rgb8(w, h).  Only the DEFLATE stream may differ, and it is a pure function of the
 * pixels and the options (filter, chain) too.
 *
 * Matches.  d[0 .. F) are the filtered bytes of one image, K = `chain` (1..MDCL_MAX_CHAIN, fixed at creation).  For a position p with
 * p + 2 < F:
 *   candidates: the K nearest earlier positions q < p with p - q <= 32768 and d[q], d[q+1], d[q+2] == d[p], d[p+1], d[p+2] (equality of
 *               the three bytes, no hash: nothing depends on a table size);
 *   cap(p)    = min(258, F - p, 4096 - p % 4096): a match never crosses a multiple of 4096;
 *   the length of a candidate = the number of leading j < cap(p) with d[q + j] == d[p + j] (q + j may pass p: the source may run into
 *               the match);
 *   best(p)   = the candidate of the greatest length, of equal lengths the nearest; it counts if its length is >= 4.
 * Positions with p + 2 >= F have no match.
 *
 * Parse, greedy from the left inside every 4096-byte chunk [4096 c, min(F, 4096 c + 4096)): at p, if best(p) counts, the token is the
 * match (length, distance = p - q) and p += length; else the token is the literal d[p] and p += 1.  No lazy evaluation.  Every chunk
 * starts a token, so the chunks parse independently.
 *
 * Codes: one dynamic block (BFINAL 1, BTYPE 2) per image.  Lengths and distances map to symbols and extra bits as RFC 1951 3.2.5 has
 * it (length 258 is symbol 285).  The literal/length histogram (286 symbols; the end-of-block counts once) and the distance
 * histogram (30 symbols) each go through the code-length rule of include/mdc_pngw.h ("Code lengths") with limit 15, and both codes
 * are canonical.  HLIT covers up to the last literal/length symbol of non-zero length, at least 257 codes; HDIST up to the last
 * distance symbol of non-zero length, at least 1 code.  With no match in the image the one distance code has length 0; with exactly
 * one distance symbol used its code has length 1 (the rule's n == 1 case).  The HLIT + HDIST code lengths are run-length coded as ONE
 * sequence by the greedy rule of include/mdc_pngw.h, the code-length code is limited to 7 bits, HCLEN as there.  A match is written as
 * length code, length extra bits, distance code, distance extra bits (extra bits as plain values, LSB-first); then the end-of-block
 * code; the stream is padded to a byte.
 *
 * Choice of form, per image, on the device.  L = the bytes of the stream above; H = the bytes of include/mdc_pngw.h's Huffman-only
 * dynamic stream of the same filtered bytes; S = F + 5 * ceil(F / 65535), the stored size.
 *   L < H and L < S: the match form (MDCL_FORM_MATCHES);  else H < S: the Huffman-only form (MDCL_FORM_HUFFMAN), the very stream of
 *   include/mdc_pngw.h;  else the stored form (MDCL_FORM_STORED), as there.
 * So a file is never larger than libmdc_pngw.so's / libmdc_pngw_rgb.so's for the same pixels and filter, and unless the match form is
 * taken it IS their file, byte for byte.  An image without a match has L == H and never takes the match form.
 *
 * Float input is converted as mdcp_encode_f32_device does: rintf (ties to even), clamped to 0..255, NaN -> 0.
 *
 * Reading.  The files are ordinary PNG.  This project's reader sends a stream with distance codes to its host decoder unless
 * MDC_GPU_PNG=2 asks for the device decoder's general path (include/mdc_pngd.h), which reads them too.
 *
 * Limits, each checked and reported as an error status (never a fault):
 *   1 <= w, h; kind MDCL_GRAY8, MDCL_GRAY16 or MDCL_RGB8; filter 0..4 or MDCL_FILTER_ADAPTIVE; 1 <= chain <= MDCL_MAX_CHAIN;
 *   mdcl_png_bound(w, h, kind) <= 2^31 - 1; 1 <= max_images; the scratch arrays, max_images * (152 * ceil(F / 16) + 4232) bytes (per 16
 *   filtered bytes: the bytes themselves 16, the positions in trigram order 64, the sorting copy that then holds every position's best
 *   match 64, a 64-bit bit offset 8; histograms and tables), at most 2^40 bytes; per call 0 <= nimages <= max_images, stride >= w * h
 *   elements (rgb8: 3 * w * h bytes), slot_bytes >= the bound, 16-bit images 2-byte aligned, float images 4-byte aligned; d_out and
 *   slot_bytes of any alignment.
 *   The ordering of an image's positions, its code builder and the scan over its bit offsets each run in one workgroup per image: the
 *   encoder is made for batches of images, not for one large image.  The parse is one lane per 4096-byte chunk.
 *
 * Threads: as include/mdc_pngw.h -- an encoder holds the scratch arrays of one call at a time; the encode calls enqueue on `stream`
 * (hipStream_t as void*, NULL = the default stream) and do not synchronise.
 */
#ifndef MDC_PNGLZ_H
#define MDC_PNGLZ_H
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

#define MDCL_OK 0
#define MDCL_ERR_ARG (-1)       /* null pointer, kind / filter / chain / nimages / stride / alignment out of range */
#define MDCL_ERR_SIZE (-3)      /* w, h, the bound or the scratch beyond the limits above; slot_bytes below the bound */
#define MDCL_ERR_HIP (-4)       /* a HIP call failed */
#define MDCL_ERR_NO_DEVICE (-5) /* no such HIP device */
#define MDCL_ERR_NOMEM (-6)     /* the scratch arrays could not be allocated */

#define MDCL_GRAY8 0
#define MDCL_GRAY16 1
#define MDCL_RGB8 2

#define MDCL_FILTER_ADAPTIVE 5
#define MDCL_MAX_CHAIN 64

#define MDCL_FORM_STORED 0
#define MDCL_FORM_HUFFMAN 1
#define MDCL_FORM_MATCHES 2

#define MDCL_KERNELS 9 /* of mdcl_kernel_ms: filter, order, match, parse, tally, build, scan, pack, finish + checksum */

typedef struct mdcl_encoder mdcl_encoder;

/* Exact size in bytes of a w x h image of `kind` in the stored form, the upper bound of every file; -1 when w or h is below 1, kind
 * is none of the three, or the result passes 2^31 - 1. */
MDC_API int64_t mdcl_png_bound(int w, int h, int kind);

/* The message of the calling thread's last failed mdcl_* call ("" if none). */
MDC_API const char* mdcl_last_error(void);

/* An encoder for images of w x h of `kind` with `filter` and match depth `chain` on HIP device `device` (-1 = the calling thread's
 * current device), with scratch arrays for up to max_images images per call. */
MDC_API int mdcl_create(int device, int w, int h, int kind, int filter, int chain, int max_images, mdcl_encoder** out);
MDC_API void mdcl_destroy(mdcl_encoder* enc);

/* nimages images, image f = w * h elements (rows of w, no padding) at d_images + f * stride (in elements)  ->  its PNG file at
 * d_out + f * slot_bytes, and the file's length in d_sizes[f].  Nothing outside [f * slot_bytes, f * slot_bytes + d_sizes[f]) is
 * written.  u8 and f32 need an encoder of kind MDCL_GRAY8, u16 one of MDCL_GRAY16. */
MDC_API int mdcl_encode_u8_device(mdcl_encoder* enc, const uint8_t* d_images, int64_t stride, int nimages, uint8_t* d_out, int64_t slot_bytes,
                                  int32_t* d_sizes, void* stream);
MDC_API int mdcl_encode_u16_device(mdcl_encoder* enc, const uint16_t* d_images, int64_t stride, int nimages, uint8_t* d_out, int64_t slot_bytes,
                                   int32_t* d_sizes, void* stream);
/* The file of mdcl_encode_u8_device on the converted values. */
MDC_API int mdcl_encode_f32_device(mdcl_encoder* enc, const float* d_images, int64_t stride, int nimages, uint8_t* d_out, int64_t slot_bytes,
                                   int32_t* d_sizes, void* stream);
/* Image f = w * h pixels of three bytes R, G, B at d_images + f * stride_bytes; an encoder of kind MDCL_RGB8. */
MDC_API int mdcl_encode_rgb8_device(mdcl_encoder* enc, const uint8_t* d_images, int64_t stride_bytes, int nimages, uint8_t* d_out, int64_t slot_bytes,
                                    int32_t* d_sizes, void* stream);

/* Output arrays owned by the encoder: max_images slots of *slot_bytes = the bound and max_images sizes, allocated on the first call
 * and freed by mdcl_destroy. */
MDC_API int mdcl_output_device(mdcl_encoder* enc, uint8_t** d_out, int64_t* slot_bytes, int32_t** d_sizes);

/* For tests and the rate tool: four int32_t per image of the encoder's last encode call into d_form[4 * nimages] (device memory),
 * copied on `stream` behind that call (the caller orders the two as it orders encode calls): the form taken (MDCL_FORM_*), the tokens
 * of the parse (literals + matches, the end-of-block not counted), its matches, and L, the bytes of the match-form stream. */
MDC_API int mdcl_form_device(mdcl_encoder* enc, int32_t* d_form, int nimages, void* stream);

/* on != 0: HIP events around the stages of every encode call from now on. */
MDC_API int mdcl_profile(mdcl_encoder* enc, int on);
/* ms[MDCL_KERNELS] of the last timed encode call, in the order given at MDCL_KERNELS; waits for that call. */
MDC_API int mdcl_kernel_ms(mdcl_encoder* enc, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* MDC_PNGLZ_H */
