/*
 * mdc_lensinv.h -- C interface of libmdc_lensinv.so: the lens models of camera.txt run backwards, on the device.
 *
 * Raw (distorted) pixel coordinates -> rectified pixel coordinates through a pinhole, a RadTan (OpenCV radial-tangential), an
 * EquiDistant (Kannala-Brandt fisheye) or a FOV (atan) camera, and the table that gives every raw pixel its place in the rectified
 * image.  It is the other half of include/mdc_lens.h (and of mdc_distort_points_* for FOV).  The arithmetic is that of
 * csrc/lens_inverse_model.h, the same header the host class runs: IEEE single precision, no FMA, a tangent of its own, Newton
 * iterations of the fixed length 8 -- the device gives the host's bits.
 *
 * Where NaN comes out (both coordinates): FOV, a raw radius rd with rd * omega not below pi/2 (the float 1.5707962513); EquiDistant,
 * a solved angle outside [0, pi/2) -- a fisheye's corners past 90 degrees --; RadTan, an iteration that left the finite numbers; and
 * NaN in.  mdcu_inverse_remap_device turns all of these into its (-1, -1) entries.
 *
 * A library of its own: it links nothing of this project, and nothing links it (libmdc_host.so loads it at run time for bulk
 * undistortCoordinates() calls; MDC_LIB_LENSINV names another file).
 *
 * Limits, each checked and reported as an error status (never a fault): kind one of MDCU_*; fx, fy, ofx, ofy finite and not 0; for
 * mdcu_inverse_remap_device 1 <= in_w, in_h, out_w, out_h and in_w * in_h < 2^31; n >= 0.  Arrays of any alignment a float allows.
 *
 * The *_device calls enqueue on `stream` (hipStream_t as void*, NULL = the default stream) of the calling thread's current device and
 * do not synchronise; mdcu_undistort_points_host blocks.
 */
#ifndef MDC_LENSINV_H
#define MDC_LENSINV_H
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

#define MDCU_OK 0
#define MDCU_ERR_ARG (-1)       /* null pointer, negative n, a model outside the limits above */
#define MDCU_ERR_SIZE (-3)      /* table or staging sizes beyond the limits above */
#define MDCU_ERR_HIP (-4)       /* a HIP call failed */
#define MDCU_ERR_NO_DEVICE (-5) /* no such HIP device */
#define MDCU_ERR_NOMEM (-6)     /* the staging arrays could not be allocated */

#define MDCU_PINHOLE 0     /* no distortion term; k unused */
#define MDCU_RADTAN 1      /* k = k1 k2 p1 p2 */
#define MDCU_EQUIDISTANT 2 /* k = k1 k2 k3 k4 (camera.txt: EquiDistant or KannalaBrandt) */
#define MDCU_FOV 3         /* k[0] = omega, the rest unused */

/* A camera pair, everything in pixels: the input (raw) camera fx fy cx cy k[4] of an in_w x in_h image and the rectified pinhole
 * camera ofx ofy ocx ocy of an out_w x out_h image -- the layout of mdcn_model (include/mdc_lens.h), 17 words.  The sizes matter to
 * mdcu_inverse_remap_device only. */
typedef struct mdcu_model {
  int kind;
  float fx, fy, cx, cy, k[4];
  int in_w, in_h;
  float ofx, ofy, ocx, ocy;
  int out_w, out_h;
} mdcu_model;

/* The message of the calling thread's last failed mdcu_* call ("" if none). */
MDC_API const char* mdcu_last_error(void);

/* n raw points (d_x[i], d_y[i]), device arrays, in place -> rectified points.  n = 0 is a no-op; NaN in gives NaN out. */
MDC_API int mdcu_undistort_points_device(const mdcu_model* model, float* d_x, float* d_y, int64_t n, void* stream);

/* The same on host arrays, blocking, on HIP device `device` (-1 = the calling thread's current device) with staging of its own.
 * When it fails the coordinates are untouched (they are copied back last). */
MDC_API int mdcu_undistort_points_host(int device, const mdcu_model* model, float* x, float* y, int64_t n);

/* The in_w x in_h inverse table of the model: for every raw pixel its rectified coordinates, then the class's border rules against
 * the OUTPUT size (an exact hit on the first / last rectified row or column is nudged inside, everything not strictly inside the
 * rectified image -- NaN included -- becomes (-1, -1)).  *d_outside (device) = 1 if any entry did, else 0.  The tables have the
 * format of the class's remap tables: mdc_set_remap(ctx, ux, uy, out_w, out_h, in_w, in_h) -- the two sizes swapped -- makes the
 * frame kernels re-distort rectified frames into the raw geometry. */
MDC_API int mdcu_inverse_remap_device(const mdcu_model* model, float* d_ux, float* d_uy, int* d_outside, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDC_LENSINV_H */
