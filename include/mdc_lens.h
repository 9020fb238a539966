/*
 * mdc_lens.h -- C interface of libmdc_lens.so: the lens models of DSO's camera.txt grammar beside FOV, on the device.
 *
 * Rectified pixel coordinates -> raw (distorted) pixel coordinates through a pinhole, a RadTan (OpenCV radial-tangential) or an
 * EquiDistant (Kannala-Brandt fisheye; DSO's names "EquiDistant" and "KannalaBrandt" are this one polynomial) camera, and the remap
 * tables of class UndistorterFOV built from such a camera.  The arithmetic is that of csrc/lens_point_model.h, the same header the host
 * class runs: IEEE single precision, no FMA, the host libm's atanf restated -- the device gives the host's bits.
 *
 * A library of its own: it links nothing of this project, and nothing links it (libmdc_host.so loads it at run time for bulk
 * distortCoordinates() calls on such cameras; MDC_LIB_LENS names another file).
 *
 * Limits, each checked and reported as an error status (never a fault): kind one of MDCN_*; ofx, ofy finite and not 0; for
 * mdcn_remap_device 1 <= in_w, in_h, out_w, out_h and out_w * out_h < 2^31; n >= 0.  Arrays of any alignment a float allows.
 *
 * The *_device calls enqueue on `stream` (hipStream_t as void*, NULL = the default stream) of the calling thread's current device and
 * do not synchronise; mdcn_distort_points_host blocks.
 */
#ifndef MDC_LENS_H
#define MDC_LENS_H
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

#define MDCN_OK 0
#define MDCN_ERR_ARG (-1)       /* null pointer, negative n, a model outside the limits above */
#define MDCN_ERR_SIZE (-3)      /* table or staging sizes beyond the limits above */
#define MDCN_ERR_HIP (-4)       /* a HIP call failed */
#define MDCN_ERR_NO_DEVICE (-5) /* no such HIP device */
#define MDCN_ERR_NOMEM (-6)     /* the staging arrays could not be allocated */

#define MDCN_PINHOLE 0     /* no distortion term; k unused */
#define MDCN_RADTAN 1      /* k = k1 k2 p1 p2 */
#define MDCN_EQUIDISTANT 2 /* k = k1 k2 k3 k4 (camera.txt: EquiDistant or KannalaBrandt) */

/* A camera pair, everything in pixels: the input (raw) camera fx fy cx cy k[4] of an in_w x in_h image and the rectified pinhole
 * camera ofx ofy ocx ocy of an out_w x out_h image.  The sizes matter to mdcn_remap_device only. */
typedef struct mdcn_model {
  int kind;
  float fx, fy, cx, cy, k[4];
  int in_w, in_h;
  float ofx, ofy, ocx, ocy;
  int out_w, out_h;
} mdcn_model;

/* The message of the calling thread's last failed mdcn_* call ("" if none). */
MDC_API const char* mdcn_last_error(void);

/* n points (d_x[i], d_y[i]), device arrays, in place.  n = 0 is a no-op; NaN in gives NaN out. */
MDC_API int mdcn_distort_points_device(const mdcn_model* model, float* d_x, float* d_y, int64_t n, void* stream);

/* The same on host arrays, blocking, on HIP device `device` (-1 = the calling thread's current device) with staging of its own.
 * When it fails the coordinates are untouched (they are copied back last). */
MDC_API int mdcn_distort_points_host(int device, const mdcn_model* model, float* x, float* y, int64_t n);

/* The out_w x out_h remap tables of the model: the identity grid through the lens, then the class's border rules (an exact hit on the
 * first / last row or column is nudged inside, everything not strictly inside the input becomes (-1, -1)).  *d_black (device) = 1 if
 * any entry became black, else 0.  The bits are those of UndistorterFOV's constructor for the same cameras. */
MDC_API int mdcn_remap_device(const mdcn_model* model, float* d_rx, float* d_ry, int* d_black, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDC_LENS_H */
