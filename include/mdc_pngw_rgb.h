/*
 * mdc_pngw_rgb.h -- C interface of libmdc_pngw_rgb.so: the device PNG encoder of mdc_pngw.h for 8-bit RGB images (the colour plots of
 * the calibration tools: E-k.png of responseCalib, plane.png of vignetteCalib).  The same translation unit as libmdc_pngw.so, built for
 * the other pixel kind: a library of its own with entry points of its own, so that the gray library -- its kernels, its exported names
 * and every file it writes -- is untouched; the two can be loaded into one process.  It links libmdc_zipw.so for mdcz_crc32_device.
 *
 * Everything mdc_pngw.h says holds with these changes.  The file: IHDR colour type 2 (truecolour) at depth 8.  A pixel is three bytes
 * R, G, B on the device, as in the file; the filter distance bpp is 3, a row is 1 + 3 w filtered bytes and F = h * (1 + 3 w).  The
 * adaptive rule, the Huffman-only block, the code builder, the stored fallback with D < S, the single IDAT and the limits are those of
 * mdc_pngw.h read with this F; mdcp_png_bound_rgb8(w, h) = 57 + 6 + S is exact for the stored form and bounds every file.  Per call
 * stride_bytes >= 3 * w * h; d_images, d_out and slot_bytes of any alignment.
 *
 * The status codes, MDCP_FILTER_ADAPTIVE and the type mdcp_encoder are mdc_pngw.h's.  An encoder made here is used with the calls
 * declared here only (the last-error message is this library's own).
 */
#ifndef MDC_PNGW_RGB_H
#define MDC_PNGW_RGB_H
#include "mdc_pngw.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Exact size in bytes of a w x h 8-bit RGB image written in the stored form, the upper bound of every file; -1 when w or h is below
 * 1 or the result passes 2^31 - 1. */
MDC_API int64_t mdcp_png_bound_rgb8(int w, int h);

/* The message of the calling thread's last failed call of this header ("" if none). */
MDC_API const char* mdcp_last_error_rgb8(void);

/* An encoder for 8-bit RGB images of w x h with `filter` on HIP device `device` (-1 = the calling thread's current device), with
 * scratch arrays for up to max_images images per call. */
MDC_API int mdcp_create_rgb8(int device, int w, int h, int filter, int max_images, mdcp_encoder** out);
MDC_API void mdcp_destroy_rgb8(mdcp_encoder* enc);

/* nimages images, image f = h rows of w pixels of three bytes R, G, B (no padding) at d_images + f * stride_bytes  ->  its PNG file at
 * d_out + f * slot_bytes, and the file's length in d_sizes[f].  Nothing outside [f * slot_bytes, f * slot_bytes + d_sizes[f]) is
 * written.  Enqueues on `stream` and does not synchronise. */
MDC_API int mdcp_encode_rgb8_device(mdcp_encoder* enc, const uint8_t* d_images, int64_t stride_bytes, int nimages, uint8_t* d_out,
                                    int64_t slot_bytes, int32_t* d_sizes, void* stream);

/* Output arrays owned by the encoder: max_images slots of *slot_bytes = mdcp_png_bound_rgb8(w, h) and max_images sizes, allocated on
 * the first call and freed by mdcp_destroy_rgb8. */
MDC_API int mdcp_output_device_rgb8(mdcp_encoder* enc, uint8_t** d_out, int64_t* slot_bytes, int32_t** d_sizes);

#ifdef __cplusplus
}
#endif
#endif /* MDC_PNGW_RGB_H */
