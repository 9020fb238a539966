/*
 * mdc_pngd.h -- C interface of libmdc_pngd.so: a PNG decoder on the device, the reading side of include/mdc_pngw.h.
 *
 * Scope: 8-bit grayscale, non-interlaced images of one size w x h per decoder -- the dataset reader's frames.  The input of a frame
 * is its ZLIB STREAM: the bodies of the file's IDAT chunks, concatenated, starting at the two header bytes (78 ..) and ending with
 * the Adler-32.  The chunk walk is the caller's (mdch_png_stream in include/mdc_host.h does it on the host); for a file with exactly
 * one IDAT that follows IHDR directly -- what mdcp_encode_*_device writes -- the stream is the file without its first 41 and its last
 * 16 bytes, which is what skip_head / skip_tail are for.  A library of its own: it links nothing of this project, nothing links it.
 *
 * A frame is F = h * (1 + w) filtered bytes (each row: its filter type 0..4, then w bytes), inflated (RFC 1950, RFC 1951), checked
 * against the stream's Adler-32 and unfiltered (PNG specification, 9.2) into w * h pixels.  Every valid DEFLATE stream is read: stored,
 * fixed and dynamic blocks, any number of them, matches at any distance.
 *
 * Paths.  A stream is decoded by one of three paths, reported with its status:
 *   MDCI_PATH_PARALLEL  a single final dynamic block in which no distance symbol has a code (every symbol is a literal or the
 *                       end-of-block: what mdcp_encode_*_device writes).  One workgroup per image; every thread decodes a
 *                       subsequence of the bits from a guessed entry position, the entry positions relax to the sequential decoder's
 *                       (at most as many rounds as there are subsequences), a prefix sum over the symbol counts gives the output
 *                       positions, a second pass writes.
 *   MDCI_PATH_STORED    stored blocks only, at most MDCI_MAX_STORED_BLOCKS of them: one lane walks the block headers, the workgroup
 *                       copies.
 *   MDCI_PATH_GENERAL   every other stream, and every stream one of the two paths above gave up on (any irregularity: the sequential
 *                       decoder has the last word, so a status never depends on the path): one wave per image, symbol by symbol;
 *                       the wave copies the matches.
 *
 * Status of a frame: d_status[f] = reason | path << 16.  reason 0: the frame's w * h pixels were written.  Otherwise nothing of the
 * frame's output is defined (no byte at or past its w * h bytes is ever written), and reason says why; what is refused is what
 * zlib's inflate refuses.  The first failure in this order is reported:
 *   the stream, in its own order: MDCI_ST_TRUNCATED (input ends inside the stream), MDCI_ST_ZLIB_HEADER, MDCI_ST_BLOCK_TYPE (3),
 *   MDCI_ST_STORED_LEN (LEN != ~NLEN), MDCI_ST_BAD_CODE (over-subscribed or incomplete code, a bad run in the code lengths, no
 *   end-of-block code), MDCI_ST_UNDEFINED_SYMBOL (bits that are no code; length symbols 286, 287; distance symbols 30, 31),
 *   MDCI_ST_DISTANCE (before the first output byte), MDCI_ST_OUTPUT_SIZE (a byte past F);
 *   then MDCI_ST_OUTPUT_SIZE (fewer than F bytes), MDCI_ST_TRUNCATED (no four bytes of trailer), MDCI_ST_ADLER, MDCI_ST_FILTER_TYPE
 *   (a row's type byte above 4).  Bytes after the trailer are ignored, as zlib's uncompress ignores them.
 *
 * Limits, each checked and reported as an error status of the call (never a fault): 1 <= w, h; F <= 2^28; 1 <= max_images; the
 * scratch (mdci_scratch_bytes) at most 2^40 bytes; per call 0 <= n <= max_images, slot_bytes >= 0, skip_head, skip_tail >= 0,
 * frame_stride >= w * h.  A stream longer than 2^29 - 1 bytes is read up to there (bit positions are 32-bit).  Slots, sizes of any
 * alignment the types allow; d_frames of any alignment.
 *
 * Threads: a decoder holds the scratch of one call at a time; calls on one decoder are ordered by the caller.  mdci_decode_device
 * enqueues on `stream` (hipStream_t as void*, NULL = the default stream) and does not synchronise; mdci_decode_host blocks.
 */
#ifndef MDC_PNGD_H
#define MDC_PNGD_H
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

#define MDCI_OK 0
#define MDCI_ERR_ARG (-1)       /* null pointer, n / stride / skip out of range */
#define MDCI_ERR_SIZE (-3)      /* w, h, F or the scratch beyond the limits above */
#define MDCI_ERR_HIP (-4)       /* a HIP call failed */
#define MDCI_ERR_NO_DEVICE (-5) /* no such HIP device */
#define MDCI_ERR_NOMEM (-6)     /* the scratch arrays could not be allocated */

#define MDCI_ST_OK 0
#define MDCI_ST_TRUNCATED 1
#define MDCI_ST_ZLIB_HEADER 2
#define MDCI_ST_BLOCK_TYPE 3
#define MDCI_ST_STORED_LEN 4
#define MDCI_ST_BAD_CODE 5
#define MDCI_ST_UNDEFINED_SYMBOL 6
#define MDCI_ST_DISTANCE 7
#define MDCI_ST_OUTPUT_SIZE 8
#define MDCI_ST_FILTER_TYPE 9
#define MDCI_ST_ADLER 10

#define MDCI_PATH_PARALLEL 1
#define MDCI_PATH_STORED 2
#define MDCI_PATH_GENERAL 3
#define MDCI_MAX_STORED_BLOCKS 64

#define MDCI_STATUS_REASON(s) ((s) & 0xffff)
#define MDCI_STATUS_PATH(s) (((s) >> 16) & 0xff)

typedef struct mdci_decoder mdci_decoder;

/* The message of the calling thread's last failed mdci_* call ("" if none). */
MDC_API const char* mdci_last_error(void);

/* The device memory a decoder of this size allocates when it is made (the filtered bytes and four words per image); -1 outside the
 * limits.  mdci_decode_host adds its own staging and output arrays on first use (the streams' bytes and max_images * w * h). */
MDC_API int64_t mdci_scratch_bytes(int w, int h, int max_images);

/* A decoder for w x h images on HIP device `device` (-1 = the calling thread's current device), up to max_images per call. */
MDC_API int mdci_create(int device, int w, int h, int max_images, mdci_decoder** out);
MDC_API void mdci_destroy(mdci_decoder* dec);

/* n frames; frame f's stream = the bytes [skip_head, d_sizes[f] - skip_tail) of the slot at d_slots + f * slot_bytes (a stream of no
 * bytes if that is empty; d_sizes[f] above slot_bytes counts as slot_bytes)  ->  its pixels at d_frames + f * frame_stride (bytes), its
 * status in d_status[f].  skip_head = 41, skip_tail = 16 read mdcp_encode_u8_device's files where it left them. */
MDC_API int mdci_decode_device(mdci_decoder* dec, const uint8_t* d_slots, int64_t slot_bytes, const int32_t* d_sizes, int skip_head, int skip_tail, int n,
                               uint8_t* d_frames, int64_t frame_stride, int32_t* d_status, void* stream);

/* The same from host memory, blocking: streams[f] of bytes[f] bytes are uploaded in one copy and decoded; status[f] as above, and
 * *d_frames = the decoder's own dense n x h x w array on the device, valid until the next call on this decoder. */
MDC_API int mdci_decode_host(mdci_decoder* dec, const void* const* streams, const int64_t* bytes, int n, int* status, const uint8_t** d_frames);

/* For measurements: with profiling on, mdci_decode_device records HIP events around its four kernels on the call's stream, and
 * mdci_kernel_ms waits for the last timed call and gives ms[0..3] = the front kernel (header, parallel and stored paths), the
 * wave-per-image inflate, the Adler-32 and checks, the unfilter.  Off by default. */
MDC_API int mdci_profile(mdci_decoder* dec, int on);
MDC_API int mdci_kernel_ms(mdci_decoder* dec, float ms[4]);

/* The stream mdci_decode_host works on (a hipStream_t of the decoder's own, made at the first call of either function; NULL on
 * failure), for consumers that read *d_frames with kernels of their own and have no HIP: enqueue them on it, then mdci_synchronize
 * waits for everything enqueued there.  The next mdci_decode_host overwrites the frames. */
MDC_API void* mdci_stream(mdci_decoder* dec);
MDC_API int mdci_synchronize(mdci_decoder* dec);

#ifdef __cplusplus
}
#endif
#endif /* MDC_PNGD_H */
