/*
 * mdc_jenc.h -- C interface of libmdc_jenc.so: a baseline JPEG encoder for device-resident grayscale frames.
 *
 * The saving mode of the reference's playDataset (src/main_playbackDataset.cpp:73-85) writes every rectified frame with
 * cv::imwrite("%05d.jpg", CV_32F image).  This library makes that file on the GPU from the float frames that
 * mdc_process_batch_device / DatasetReader::getImagesDevice leave in device memory, so that only the encoded bytes cross
 * PCIe.  A library of its own: libmdc_hip.so / libmdc_host.so neither link nor load it, and it needs no mdc_ctx.
 *
 * What is written, per frame, is the file libjpeg writes for an 8-bit one-component image at the given quality with default
 * settings (what cv::imwrite and PIL's Image.save(..., 'JPEG', quality=Q) call), byte for byte:
 *   - float -> 8 bit as cv::Mat::convertTo(CV_8U): rintf (ties to even), clamped to 0..255, NaN -> 0.  Values with
 *     |v| >= 2^31 are outside that contract (x86 cvRound gives INT_MIN for them, so OpenCV writes 0 also for the positive
 *     ones); here they are clamped like every other value: -> 0 or 255 by their sign.
 *   - the last column / row repeated up to a multiple of 8; level shift by -128; the forward DCT of jfdctint.c in 32-bit
 *     integers (CONST_BITS 13, PASS1_BITS 2; rows, then columns; output scaled by 8); quantisation as jcdctmgr.c:
 *     (|c| + d/2) / d with d = 8 q[i], sign restored; q = (Annex K luminance * scale + 50) / 100 clamped to 1..255, scale =
 *     5000 / Q below 50, else 200 - 2 Q.
 *   - baseline sequential Huffman coding with the Annex K luminance tables, no restart interval; 0x00 after every 0xFF; the
 *     last byte padded with 1-bits; SOI, JFIF APP0 (1.01, unit 0, density 1:1), DQT, SOF0, DHT (DC), DHT (AC), SOS in front, EOI
 *     behind.
 *
 * Slot size.  mdcj_jpeg_bound(w, h) = 1024 + 416 * B with B = ceil(w/8) * ceil(h/8) blocks is an upper bound of the file:
 *   a block is coded as one DC symbol (code <= 9 bits + <= 11 amplitude bits = 20) and at most 63 AC symbols (code <= 16 bits
 *   + <= 10 amplitude bits = 26; ZRL and EOB only replace coefficients, so 63 coded coefficients is the longest form): at most
 *   20 + 63 * 26 = 1658 bits.  The scan has at most ceil(1658 B / 8) <= 208 B bytes before stuffing, and at most twice that
 *   after (every byte 0xFF): 416 B.  The headers are 328 bytes and EOI is 2: below 1024.
 *
 * Limits, each checked and reported as an error status (never a fault):
 *   1 <= w, h <= 65535 (the 16-bit SOF0 fields); 1 <= quality <= 100; mdcj_jpeg_bound(w, h) <= 2^30 (a frame's bit offsets are
 *   32-bit: 2.58 million blocks, 165 megapixels); 1 <= max_frames, and blocks * max_frames < 2^31; per call 0 <= nframes <=
 *   max_frames, frame_stride >= w * h elements, slot_bytes >= mdcj_jpeg_bound(w, h).  Offsets across the batch (frame_stride *
 *   frame, slot_bytes * frame) are 64-bit.
 *
 * Threads: an encoder holds the scratch arrays of one call at a time -- calls on one encoder are ordered by the caller (same
 * stream, or synchronised); different encoders are independent.  The encode calls enqueue on `stream` (hipStream_t as void*,
 * NULL = the default stream) and do not synchronise.
 */
#ifndef MDC_JENC_H
#define MDC_JENC_H
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

#define MDCJ_OK 0
#define MDCJ_ERR_ARG (-1)       /* null pointer, quality / nframes / stride out of range */
#define MDCJ_ERR_SIZE (-3)      /* w, h or the bound beyond the limits above; slot_bytes below the bound */
#define MDCJ_ERR_HIP (-4)       /* a HIP call failed */
#define MDCJ_ERR_NO_DEVICE (-5) /* no such HIP device */
#define MDCJ_ERR_NOMEM (-6)     /* the scratch arrays could not be allocated */

typedef struct mdcj_encoder mdcj_encoder;

/* Upper bound in bytes of one encoded w x h frame (derivation above); -1 when w or h is outside 1..65535. */
MDC_API int64_t mdcj_jpeg_bound(int w, int h);

/* The message of the calling thread's last failed mdcj_* call ("" if none). */
MDC_API const char* mdcj_last_error(void);

/* An encoder for frames of w x h at `quality` on HIP device `device` (-1 = the calling thread's current device), with
 * scratch arrays for up to max_frames frames per call: (128 + 4 + 208) bytes per block and frame. */
MDC_API int mdcj_create(int device, int w, int h, int quality, int max_frames, mdcj_encoder** out);
MDC_API void mdcj_destroy(mdcj_encoder* enc);

/* nframes frames, frame f = w * h floats (rows of w, no padding) at d_frames + f * frame_stride  ->  its JPEG file at d_out + f *
 * slot_bytes, and the file's length in d_sizes[f].  Nothing outside [f * slot_bytes, f * slot_bytes + d_sizes[f]) is written. */
MDC_API int mdcj_encode_f32_device(mdcj_encoder* enc, const float* d_frames, int64_t frame_stride, int nframes, uint8_t* d_out,
                                   int64_t slot_bytes, int32_t* d_sizes, void* stream);
/* The same for 8-bit frames (everything after the conversion is shared): the file of mdcj_encode_f32_device on the same values. */
MDC_API int mdcj_encode_u8_device(mdcj_encoder* enc, const uint8_t* d_frames, int64_t frame_stride, int nframes, uint8_t* d_out,
                                  int64_t slot_bytes, int32_t* d_sizes, void* stream);

/* Output arrays owned by the encoder, for callers without an allocator of their own: max_frames slots of *slot_bytes =
 * mdcj_jpeg_bound(w, h) and max_frames sizes, allocated on the first call and freed by mdcj_destroy. */
MDC_API int mdcj_output_device(mdcj_encoder* enc, uint8_t** d_out, int64_t* slot_bytes, int32_t** d_sizes);

/* After an encode call on `stream`: the nframes sizes into h_sizes, then -- unless h_out is NULL -- every file's bytes (and only
 * those: d_sizes[f] bytes of slot f) back to back into h_out, file f at the sum of the sizes before it; waits for the stream.
 * The files are gathered on the device first (into an array the encoder keeps and grows on demand) and come over in one copy:
 * page-locked h_out makes that copy run at the link's rate.
 * Returns the total number of bytes, or a negative status (MDCJ_ERR_SIZE: h_capacity is smaller than the total). */
MDC_API int64_t mdcj_fetch(mdcj_encoder* enc, const uint8_t* d_out, int64_t slot_bytes, const int32_t* d_sizes, int nframes, uint8_t* h_out,
                           int64_t h_capacity, int32_t* h_sizes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDC_JENC_H */
