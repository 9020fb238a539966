/*
 * mdc_pngdx.h -- C interface of libmdc_pngdx.so: the device PNG decoder of include/mdc_pngd.h with a parallel inflate for ordinary
 * DEFLATE streams -- Huffman-coded blocks with matches, any number of them, fixed or dynamic, stored blocks between them: what zlib,
 * PIL, libpng, OpenCV and mdcl_encode_*_device (include/mdc_pnglz.h) write.  A library of its own: it links nothing of this project,
 * nothing links it, libmdc_pngd.so stays what it is.
 *
 * The interface is mdc_pngd.h's, function for function and argument for argument, with mdcx_ for mdci_.  The same scope: 8-bit
 * grayscale, non-interlaced images of one size w x h per decoder.  The same input: a frame's ZLIB STREAM (the bodies of the file's
 * IDAT chunks, concatenated, from the two header bytes to the Adler-32), found in a slot through skip_head / skip_tail.  The same
 * result: F = h * (1 + w) filtered bytes are inflated, checked against the stream's Adler-32 and unfiltered into w * h pixels.
 *
 * Paths.  d_status[f] = reason | path << 16.
 *   MDCX_PATH_PARALLEL  exactly the streams MDCI_PATH_PARALLEL takes: a single final dynamic block without a distance code.
 *   MDCX_PATH_STORED    exactly the streams MDCI_PATH_STORED takes: at most MDCX_MAX_STORED_BLOCKS stored blocks and nothing else.
 *   MDCX_PATH_TOKENS    every other stream first.  It gives up on no valid stream.
 *   MDCX_PATH_GENERAL   the sequential decoder, one wave per image: only what the token path gave up on, which is only what is not a
 *                       valid stream of F bytes.  It decodes from the start and names the reason, so a reason never depends on the
 *                       path.  A frame that the token path inflated and whose Adler-32, trailer or filter types are then refused is
 *                       reported with this path too: MDCX_PATH_TOKENS is only ever the path of a frame that was written.
 *
 * The token path, in full.  One workgroup of 1024 threads per image, nothing shared between workgroups, no waiting on another
 * workgroup, no spin: every loop below has a bound that the stream's length gives.
 *   Blocks.  From bit 16 of the stream, block by block: one thread reads the three header bits; block type 3, a stored block whose LEN is
 *     not ~NLEN or that runs past the input or past F, a dynamic header that RFC 1951 or zlib refuses: give up.  A stored block is
 *     copied by the workgroup and decoding goes on behind it, any number of times.  A Huffman block's two codes are built in LDS (the
 *     fixed codes for type 1) and its tokens are decoded window by window from its first data bit.  A block may be empty; it may end on
 *     the stream's last bit.  The final block's end, rounded up to a byte, is where the trailer starts.
 *   Windows.  A window is 65536 bits from a token boundary (fewer at the end of the input): thread t owns the subsequence of bits
 *     [64 t, 64 t + 64).  A thread decodes WHOLE TOKENS -- a literal, the end-of-block code, or length code + extra bits + distance
 *     code + extra bits, at most 48 bits -- from its entry position for as long as a token starts inside its subsequence.  Its exit
 *     state is the bit position of the first token that starts at or behind the subsequence's end (always inside the next
 *     subsequence), or END (it read the end-of-block code; the bit behind it is kept), or ERROR (bits that are no code, a length
 *     symbol above 285, a distance symbol above 29, input ending inside a token).  An entry is always a token boundary: there is no
 *     "next is a distance" state.
 *   Relaxation.  Subsequence 0 enters at the window's first bit, which is right; every other one guesses its own first bit.  In a
 *     round every subsequence whose left neighbour's exit is a bit position other than its entry decodes again from there.  A
 *     neighbour's END or ERROR is not taken over: a wrong guess often decodes to ERROR where there are distance codes, and the
 *     subsequences behind it may hold the right states already.  After round k subsequence k holds the sequential decoder's state
 *     unless one before it ended in END or ERROR, so there are at most as many rounds as subsequences, and the rounds end when one
 *     changes nothing: a code that does not synchronise costs rounds, never the path.  Then every entry is its left neighbour's exit
 *     from subsequence 0 up to the first subsequence that ended in END or ERROR, which therefore holds the sequential decoder's
 *     state: ERROR there: give up; END: the block ends there, the subsequences behind it were decoded with the wrong codes and
 *     count for nothing, the next block starts at the kept bit.  Neither: the last exit is the next window's first bit; if the
 *     input has no such bit: give up.
 *   Positions.  Every thread counts the output bytes of its tokens (1 for a literal, the length for a match); a prefix sum over the
 *     workgroup gives every thread its output position, and the window's total is checked against F before any byte is written.
 *   Writing.  The threads decode their tokens once more.  A literal goes straight to its position p, and a per-byte source index
 *     (four more bytes of scratch per filtered byte) gets src[p] = p.  Byte i of a match at q with distance d gets
 *     src[q + i] = q - d + i % d: a byte from before the match, which is what the sequential copy gives also where d is below the
 *     length.  A distance above q: give up.  Then pointer doubling: a byte whose source lies in this window and is no literal takes
 *     its source's source, all bytes at once, a barrier after each round, until nothing changes.  Sources before the window --
 *     earlier windows, earlier blocks, stored bytes -- are final.  A chain has at most one link per match of the window, a window at
 *     most 2^15 matches: at most 16 rounds, for a constant image (one chain through every match) as for any other; windows without a
 *     match skip this.  One gather then copies every match byte from its source.  Bytes written by one wave and read by another are
 *     ordered by a workgroup-scope fence and the barrier.
 *   The end.  After the final block F bytes must have been written, else: give up.  Giving up leaves the frame to the general path.
 *
 * Status of a frame: reason 0: the frame's w * h pixels were written.  Otherwise nothing of the frame's output is defined (no byte
 * at or past its w * h bytes is ever written), and reason says why, with the codes and the order of precedence of include/mdc_pngd.h:
 *   the stream, in its own order: MDCX_ST_TRUNCATED, MDCX_ST_ZLIB_HEADER, MDCX_ST_BLOCK_TYPE, MDCX_ST_STORED_LEN, MDCX_ST_BAD_CODE,
 *   MDCX_ST_UNDEFINED_SYMBOL, MDCX_ST_DISTANCE, MDCX_ST_OUTPUT_SIZE (a byte past F);
 *   then MDCX_ST_OUTPUT_SIZE (fewer than F bytes), MDCX_ST_TRUNCATED (no four bytes of trailer), MDCX_ST_ADLER, MDCX_ST_FILTER_TYPE.
 *
 * Limits, each checked and reported as an error status of the call (never a fault): 1 <= w, h; F <= 2^28; 1 <= max_images; the
 * scratch (mdcx_scratch_bytes) at most 2^40 bytes; per call 0 <= n <= max_images, slot_bytes >= 0, skip_head, skip_tail >= 0,
 * frame_stride >= w * h.  A stream longer than 2^29 - 1 bytes is read up to there.  Slots, sizes of any alignment the types allow;
 * d_frames of any alignment.
 *
 * Threads: a decoder holds the scratch of one call at a time; calls on one decoder are ordered by the caller.  mdcx_decode_device
 * enqueues on `stream` (hipStream_t as void*, NULL = the default stream) and does not synchronise; mdcx_decode_host blocks.
 */
#ifndef MDC_PNGDX_H
#define MDC_PNGDX_H
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

#define MDCX_OK 0
#define MDCX_ERR_ARG (-1)       /* null pointer, n / stride / skip out of range */
#define MDCX_ERR_SIZE (-3)      /* w, h, F or the scratch beyond the limits above */
#define MDCX_ERR_HIP (-4)       /* a HIP call failed */
#define MDCX_ERR_NO_DEVICE (-5) /* no such HIP device */
#define MDCX_ERR_NOMEM (-6)     /* the scratch arrays could not be allocated */

#define MDCX_ST_OK 0
#define MDCX_ST_TRUNCATED 1
#define MDCX_ST_ZLIB_HEADER 2
#define MDCX_ST_BLOCK_TYPE 3
#define MDCX_ST_STORED_LEN 4
#define MDCX_ST_BAD_CODE 5
#define MDCX_ST_UNDEFINED_SYMBOL 6
#define MDCX_ST_DISTANCE 7
#define MDCX_ST_OUTPUT_SIZE 8
#define MDCX_ST_FILTER_TYPE 9
#define MDCX_ST_ADLER 10

#define MDCX_PATH_PARALLEL 1
#define MDCX_PATH_STORED 2
#define MDCX_PATH_GENERAL 3
#define MDCX_PATH_TOKENS 4
#define MDCX_MAX_STORED_BLOCKS 64 /* of MDCX_PATH_STORED only: the token path copies any number of stored blocks */

#define MDCX_STATUS_REASON(s) ((s) & 0xffff)
#define MDCX_STATUS_PATH(s) (((s) >> 16) & 0xff)

typedef struct mdcx_decoder mdcx_decoder;

/* The message of the calling thread's last failed mdcx_* call ("" if none). */
MDC_API const char* mdcx_last_error(void);

/* The device memory a decoder of this size allocates when it is made (per image the filtered bytes, a 32-bit source index for each of
 * them and four words); -1 outside the limits.  mdcx_decode_host adds its own staging and output arrays on first use. */
MDC_API int64_t mdcx_scratch_bytes(int w, int h, int max_images);

/* A decoder for w x h images on HIP device `device` (-1 = the calling thread's current device), up to max_images per call. */
MDC_API int mdcx_create(int device, int w, int h, int max_images, mdcx_decoder** out);
MDC_API void mdcx_destroy(mdcx_decoder* dec);

/* n frames; frame f's stream = the bytes [skip_head, d_sizes[f] - skip_tail) of the slot at d_slots + f * slot_bytes (a stream of no
 * bytes if that is empty; d_sizes[f] above slot_bytes counts as slot_bytes)  ->  its pixels at d_frames + f * frame_stride (bytes), its
 * status in d_status[f].  skip_head = 41, skip_tail = 16 read mdcl_encode_u8_device's files where it left them. */
MDC_API int mdcx_decode_device(mdcx_decoder* dec, const uint8_t* d_slots, int64_t slot_bytes, const int32_t* d_sizes, int skip_head, int skip_tail, int n,
                               uint8_t* d_frames, int64_t frame_stride, int32_t* d_status, void* stream);

/* The same from host memory, blocking: streams[f] of bytes[f] bytes are uploaded in one copy and decoded; status[f] as above, and
 * *d_frames = the decoder's own dense n x h x w array on the device, valid until the next call on this decoder. */
MDC_API int mdcx_decode_host(mdcx_decoder* dec, const void* const* streams, const int64_t* bytes, int n, int* status, const uint8_t** d_frames);

/* For measurements: with profiling on, mdcx_decode_device records HIP events around its kernels on the call's stream, and
 * mdcx_kernel_ms waits for the last timed call and gives ms[0..4] = the front kernel (header, parallel and stored paths), the token
 * path, the wave-per-image inflate, the Adler-32 and checks, the unfilter.  Off by default. */
MDC_API int mdcx_profile(mdcx_decoder* dec, int on);
MDC_API int mdcx_kernel_ms(mdcx_decoder* dec, float ms[5]);

/* The stream mdcx_decode_host works on (a hipStream_t of the decoder's own, made at the first call of either function; NULL on
 * failure), for consumers that read *d_frames with kernels of their own and have no HIP: enqueue them on it, then mdcx_synchronize
 * waits for everything enqueued there.  The next mdcx_decode_host overwrites the frames. */
MDC_API void* mdcx_stream(mdcx_decoder* dec);
MDC_API int mdcx_synchronize(mdcx_decoder* dec);

#ifdef __cplusplus
}
#endif
#endif /* MDC_PNGDX_H */
