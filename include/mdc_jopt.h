/*
 * mdc_jopt.h -- C interface of libmdc_jopt.so: the JPEG encoder of mdc_jenc.h with Huffman tables made for each frame.
 *
 * libmdc_jenc.so writes every frame with the fixed Annex K tables.  This library writes the smaller file libjpeg writes with
 * optimize_coding = TRUE (PIL: Image.save(..., 'JPEG', quality=Q, optimize=True); OpenCV: IMWRITE_JPEG_OPTIMIZE), byte for byte:
 * the pixels a decoder gets are the same, the file is 3 .. 33 % smaller (8 .. 21 % on camera-like content at quality 95).  A
 * library of its own beside libmdc_jenc.so, which stays what it is: neither links the other, and nothing of libmdc_hip.so /
 * libmdc_host.so links or loads this one.  It mirrors mdc_jenc.h function by function (prefix mdcjo_); arguments, status codes
 * and threading rules are the same.
 *
 * What is written, per frame:
 *   - the quantised coefficients of mdc_jenc.h, unchanged: float -> 8 bit as cv::Mat::convertTo(CV_8U), edge extension, level
 *     shift, the forward DCT of jfdctint.c, the quantisation of jcdctmgr.c with the Annex K luminance table scaled by the quality.
 *   - one DC and one AC Huffman table per frame, built from that frame's symbol counts by the rule of jpeg_gen_optimal_table
 *     (jchuff.c of libjpeg 6b / libjpeg-turbo): a pseudo-symbol 256 of count 1 reserves the all-ones code; the two least frequent
 *     symbols are merged until one tree is left, where among equal counts the largest symbol wins and the second search leaves
 *     out the first's winner; every symbol of a merged tree gets one bit longer; lengths above 16 are folded back as in Annex
 *     K.3; the pseudo-symbol's code point is removed from the longest length; the symbols are listed by (length before folding,
 *     value).  Frame f's tables come from frame f alone.
 *   - each DHT segment lists only the symbols the frame uses, so its length varies: 19 + n bytes after the marker for n symbols.
 *   - the marker order of mdc_jenc.h: SOI, JFIF APP0, DQT, SOF0, DHT (DC), DHT (AC), SOS, the scan (0x00 after every 0xFF, the
 *     last byte padded with 1-bits), EOI.
 *
 * Two rules of libjpeg that bear on the table:
 *   - its searches look only at counts <= 1,000,000,000.  A frame has at most 64 symbols per block and mdcjo_create bounds the
 *     blocks at 2.57 million, so no count of a frame passes 165 million, and no sum of them does.
 *   - it aborts when a code is deeper than 32 before folding (JERR_HUFF_CLEN_OVERFLOW).  Here such a table gets status 1, and a
 *     frame with such a table is written with the Annex K tables -- the file of libmdc_jenc.so -- never as a fault.  Depth 33
 *     needs counts that grow like the Fibonacci numbers over 34 symbols, which no image gives;
 *     it is reachable through mdcjo_optimal_tables_device, which is how it is tested.
 *
 * Slot size.  mdcjo_jpeg_bound(w, h) = 1024 + 418 * B with B = ceil(w/8) * ceil(h/8) blocks is an upper bound of the file:
 *   a Huffman code of this format is at most 16 bits, for the DC table as for the AC table (the Annex K DC codes are at most 9;
 *   an optimal DC table has at most 12 symbols and the pseudo-symbol, so in fact at most 12 bits -- 16 is what is provisioned).
 *   A block is one DC symbol (<= 16 + 11 amplitude bits = 27) and at most 63 AC symbols (<= 16 + 10 = 26 each): at most 27 +
 *   63 * 26 = 1665 bits, where mdc_jenc.h has 1658.  The scan has at most ceil(1665 B / 8) <= 209 B bytes before stuffing and at
 *   most twice that after: 418 B.  The headers are at most 102 + (21 + 12) + (21 + 162) + 10 = 328 bytes -- 8-bit pixels reach at
 *   most 12 DC symbols and 162 AC symbols (16 runs x 10 sizes, ZRL, EOB) -- and EOI is 2: below 1024.
 *   Bit offsets: 1665 < 4 * 418, so a frame's stream has fewer than 4 * bound bits, and the rule bound <= 2^30 keeps every bit
 *   offset below 2^32 (at the limit, B = 2,568,757 blocks and 1665 B = 4,276,980,405 < 4,294,967,296).
 *   The scratch stream of a frame is sized from the same 1665 bits per block.
 *
 * Limits, each checked and reported as an error status (never a fault): those of mdc_jenc.h with this bound.
 *   1 <= w, h <= 65535; 1 <= quality <= 100; mdcjo_jpeg_bound(w, h) <= 2^30; 1 <= max_frames, and blocks * max_frames < 2^31; per
 *   call 0 <= nframes <= max_frames, frame_stride >= w * h elements, slot_bytes >= mdcjo_jpeg_bound(w, h).
 *
 * Threads: an encoder holds the scratch arrays of one call at a time -- calls on one encoder are ordered by the caller (same
 * stream, or synchronised); different encoders are independent.  The encode calls and mdcjo_optimal_tables_device enqueue on
 * `stream` (hipStream_t as void*, NULL = the default stream) and do not synchronise.
 */
#ifndef MDC_JOPT_H
#define MDC_JOPT_H
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

#define MDCJO_OK 0
#define MDCJO_ERR_ARG (-1)       /* null pointer, quality / nframes / stride / ntables out of range */
#define MDCJO_ERR_SIZE (-3)      /* w, h or the bound beyond the limits above; slot_bytes below the bound */
#define MDCJO_ERR_HIP (-4)       /* a HIP call failed */
#define MDCJO_ERR_NO_DEVICE (-5) /* no such HIP device */
#define MDCJO_ERR_NOMEM (-6)     /* the scratch arrays could not be allocated */

/* The stages mdcjo_kernel_ms reports, in the order they run. */
#define MDCJO_KERNELS 7
#define MDCJO_K_DCT 0       /* pixels -> quantised coefficients */
#define MDCJO_K_HISTOGRAM 1 /* clearing and filling the frames' symbol counts */
#define MDCJO_K_TABLES 2    /* the frames' tables and DHT segments */
#define MDCJO_K_COUNT 3     /* bits per block */
#define MDCJO_K_SCAN 4      /* bit offsets */
#define MDCJO_K_PACK 5      /* code words */
#define MDCJO_K_STUFF 6     /* headers, byte stuffing, EOI */

typedef struct mdcjo_encoder mdcjo_encoder;

/* Upper bound in bytes of one encoded w x h frame (derivation above); -1 when w or h is outside 1..65535. */
MDC_API int64_t mdcjo_jpeg_bound(int w, int h);

/* The message of the calling thread's last failed mdcjo_* call ("" if none). */
MDC_API const char* mdcjo_last_error(void);

/* An encoder for frames of w x h at `quality` on HIP device `device` (-1 = the calling thread's current device), with
 * scratch arrays for up to max_frames frames per call: (128 + 4 + 209) bytes per block and 3.7 KB per frame. */
MDC_API int mdcjo_create(int device, int w, int h, int quality, int max_frames, mdcjo_encoder** out);
MDC_API void mdcjo_destroy(mdcjo_encoder* enc);

/* nframes frames, frame f = w * h floats (rows of w, no padding) at d_frames + f * frame_stride  ->  its JPEG file at d_out + f *
 * slot_bytes, and the file's length in d_sizes[f].  Nothing outside [f * slot_bytes, f * slot_bytes + d_sizes[f]) is written. */
MDC_API int mdcjo_encode_f32_device(mdcjo_encoder* enc, const float* d_frames, int64_t frame_stride, int nframes, uint8_t* d_out,
                                    int64_t slot_bytes, int32_t* d_sizes, void* stream);
/* The same for 8-bit frames (everything after the conversion is shared): the file of mdcjo_encode_f32_device on the same values. */
MDC_API int mdcjo_encode_u8_device(mdcjo_encoder* enc, const uint8_t* d_frames, int64_t frame_stride, int nframes, uint8_t* d_out,
                                   int64_t slot_bytes, int32_t* d_sizes, void* stream);

/* Output arrays owned by the encoder, for callers without an allocator of their own: max_frames slots of *slot_bytes =
 * mdcjo_jpeg_bound(w, h) and max_frames sizes, allocated on the first call and freed by mdcjo_destroy. */
MDC_API int mdcjo_output_device(mdcjo_encoder* enc, uint8_t** d_out, int64_t* slot_bytes, int32_t** d_sizes);

/* After an encode call on `stream`: the nframes sizes into h_sizes, then -- unless h_out is NULL -- every file's bytes (and only
 * those: d_sizes[f] bytes of slot f) back to back into h_out, file f at the sum of the sizes before it; waits for the stream.
 * The files are gathered on the device first (into an array the encoder keeps and grows on demand) and come over in one copy.
 * Returns the total number of bytes, or a negative status (MDCJO_ERR_SIZE: h_capacity is smaller than the total). */
MDC_API int64_t mdcjo_fetch(mdcjo_encoder* enc, const uint8_t* d_out, int64_t slot_bytes, const int32_t* d_sizes, int nframes, uint8_t* h_out,
                            int64_t h_capacity, int32_t* h_sizes, void* stream);

/* The table rule on its own.  d_freq: ntables histograms of 257 uint32 counts each (entry 256 is ignored: the pseudo-symbol's
 * count is 1) -> per table t: d_bits[16 t ..] the number of codes of length 1..16, d_vals[256 t ..] the symbols in code order
 * (d_nvals[t] of them, the rest 0), and d_status[t]: 0 built, 1 not built -- a code deeper than 32 before folding (or, outside
 * what a frame can give, counts above 1,000,000,000 that libjpeg's search never merges); then bits and nvals are 0.  An
 * all-zero histogram gives no symbols and status 0.  Of the encoder only its device is used. */
MDC_API int mdcjo_optimal_tables_device(mdcjo_encoder* enc, const uint32_t* d_freq, int ntables, uint8_t* d_bits, uint8_t* d_vals,
                                        int32_t* d_nvals, uint8_t* d_status, void* stream);

/* Measurement (tools/jopt_rate.py): with on != 0 every encode call records HIP events around its stages, and mdcjo_kernel_ms
 * waits for the last timed call and gives their MDCJO_KERNELS times in milliseconds.  Off by default; no effect on the files. */
MDC_API int mdcjo_profile(mdcjo_encoder* enc, int on);
MDC_API int mdcjo_kernel_ms(mdcjo_encoder* enc, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* MDC_JOPT_H */
