// codec_host.h -- the host-side helpers every device codec library has (libmdc_jenc.so, libmdc_jopt.so, libmdc_zipw.so, libmdc_pngw.so,
// libmdc_pngw_rgb.so, libmdc_pnglz.so, libmdc_pngd.so, libmdc_pngdx.so) and the two lens point libraries (libmdc_lens.so,
// libmdc_lensinv.so) have: the thread's last error message, the guard that makes a call run on its object's device, and the device
// resolution of the *_create calls.  Host only.  Each library is one translation unit and includes this once (through its core
// header; the lens libraries through lens_points_shell.h); everything is in its unnamed namespace, so each library has its own
// g_error and none exports any of it.
//
// The message buffer is 320 bytes in every library.  It was 320 in libmdc_zipw.so (whose messages carry errno's text) and 256 in
// the others: no message that fitted before is cut, and one that was cut at 255 characters may now be longer.
#ifndef MDC_CODEC_HOST_H
#define MDC_CODEC_HOST_H

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

namespace {

thread_local char g_error[320] = "";

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
  return code;
}

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (dev < 0) return;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
    else prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// The status codes the libraries' public headers have in common (MDC*_OK, MDC*_ERR_*): each library asserts its own against these.
constexpr int kOk = 0, kErrArg = -1, kErrSize = -3, kErrHip = -4, kErrNoDevice = -5, kErrNoMem = -6;

// *_create's device argument: an ordinal below the device count, or negative for the calling thread's current device, which is
// written back to *device.  `who`: the caller's name, for the message.  (inline: libmdc_zipw.so has no use for it.)
inline int resolve_device(const char* who, int* device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return fail(kErrNoDevice, "%s: no HIP device", who);
  if (*device >= count) return fail(kErrNoDevice, "%s: device %d of %d", who, *device, count);
  if (*device < 0 && hipGetDevice(device) != hipSuccess) return fail(kErrHip, "%s: hipGetDevice failed", who);
  return kOk;
}

}  // namespace

#endif  // MDC_CODEC_HOST_H
