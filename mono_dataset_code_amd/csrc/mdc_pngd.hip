// libmdc_pngd.so (include/mdc_pngd.h): PNG frames decoded on the device.  One translation unit; it shares png_inflate_core.h with
// the CPU test program, and its kernels and host helpers (png_decode_kernels.h) with mdc_pngdx.hip, which is a library of its own.
//
// One call is the four kernels of png_decode_kernels.h, with no host round trip between them: front, general, check, unfilter.
#include "../../include/mdc_pngd.h"

#include <new>

#include "png_decode_kernels.h"

static_assert(MDCI_ST_TRUNCATED == pngd::ST_TRUNCATED && MDCI_ST_ZLIB_HEADER == pngd::ST_ZLIB_HEADER && MDCI_ST_BLOCK_TYPE == pngd::ST_BLOCK_TYPE &&
                  MDCI_ST_STORED_LEN == pngd::ST_STORED_LEN && MDCI_ST_BAD_CODE == pngd::ST_BAD_CODE && MDCI_ST_UNDEFINED_SYMBOL == pngd::ST_UNDEFINED_SYMBOL &&
                  MDCI_ST_DISTANCE == pngd::ST_DISTANCE && MDCI_ST_OUTPUT_SIZE == pngd::ST_OUTPUT_SIZE && MDCI_ST_FILTER_TYPE == pngd::ST_FILTER_TYPE &&
                  MDCI_ST_ADLER == pngd::ST_ADLER && MDCI_PATH_PARALLEL == pngd::PATH_PARALLEL && MDCI_PATH_STORED == pngd::PATH_STORED &&
                  MDCI_PATH_GENERAL == pngd::PATH_GENERAL && MDCI_MAX_STORED_BLOCKS == pngd::kMaxStoredBlocks,
              "include/mdc_pngd.h and png_inflate_core.h name the same codes");

struct mdci_decoder {
  int device = -1, w = 0, h = 0, max_images = 0;
  long long F = 0, filt_stride = 0;
  uint8_t* d_filt = nullptr;
  uint32_t* d_meta = nullptr;
  // mdci_decode_host: made at its first call
  hipStream_t stream = nullptr;
  uint8_t* h_stage = nullptr;  // pinned: n sizes (padded to 16 bytes), then n slots
  uint8_t* d_stage = nullptr;
  size_t stage_bytes = 0;
  uint8_t* d_out = nullptr;
  int32_t* d_status = nullptr;
  // mdci_profile: events around the four kernels of a call
  bool profile = false, timed = false;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};

extern "C" {

const char* mdci_last_error(void) { return g_error; }

int64_t mdci_scratch_bytes(int w, int h, int max_images) {
  if (w < 1 || h < 1 || max_images < 1) return -1;
  if ((1ll + w) > (1ll << 28) / h) return -1;
  const long long per_image = filt_stride_of(w, h) + 4 * kMetaWords;
  if (per_image > (1ll << 40) / max_images) return -1;
  return per_image * max_images;
}

void mdci_destroy(mdci_decoder* d) {
  if (!d) return;
  {
    DeviceGuard dg(d->device);
    if (d->stream) (void)hipStreamSynchronize(d->stream);
    (void)hipFree(d->d_filt);
    (void)hipFree(d->d_meta);
    (void)hipFree(d->d_stage);
    (void)hipFree(d->d_out);
    (void)hipFree(d->d_status);
    if (d->h_stage) (void)hipHostFree(d->h_stage);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    for (hipEvent_t e : d->ev)
      if (e) (void)hipEventDestroy(e);
  }
  delete d;
}

int mdci_create(int device, int w, int h, int max_images, mdci_decoder** out) {
  if (!out) return fail(MDCI_ERR_ARG, "mdci_create: out is null");
  *out = nullptr;
  if (max_images < 1) return fail(MDCI_ERR_ARG, "mdci_create: max_images %d is below 1", max_images);
  if (w < 1 || h < 1) return fail(MDCI_ERR_SIZE, "mdci_create: %d x %d: width and height start at 1", w, h);
  if ((1ll + w) > (1ll << 28) / h) return fail(MDCI_ERR_SIZE, "mdci_create: a %d x %d image has more than 2^28 filtered bytes", w, h);
  const int64_t scratch = mdci_scratch_bytes(w, h, max_images);
  if (scratch < 0) return fail(MDCI_ERR_SIZE, "mdci_create: %d images of %d x %d: the scratch passes 2^40 bytes", max_images, w, h);
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return fail(MDCI_ERR_NO_DEVICE, "mdci_create: no HIP device");
  if (device >= count) return fail(MDCI_ERR_NO_DEVICE, "mdci_create: device %d of %d", device, count);
  if (device < 0 && hipGetDevice(&device) != hipSuccess) return fail(MDCI_ERR_HIP, "mdci_create: hipGetDevice failed");
  DeviceGuard dg(device);
  mdci_decoder* d = new (std::nothrow) mdci_decoder;
  if (!d) return fail(MDCI_ERR_NOMEM, "mdci_create: out of host memory");
  d->device = device, d->w = w, d->h = h, d->max_images = max_images;
  d->F = (1ll + w) * h, d->filt_stride = filt_stride_of(w, h);
  if (hipMalloc((void**)&d->d_filt, (size_t)d->filt_stride * (size_t)max_images) != hipSuccess ||
      hipMalloc((void**)&d->d_meta, (size_t)max_images * kMetaWords * 4) != hipSuccess) {
    (void)hipGetLastError();
    mdci_destroy(d);
    return fail(MDCI_ERR_NOMEM, "mdci_create: could not allocate the scratch arrays of %d images of %d x %d", max_images, w, h);
  }
  *out = d;
  return MDCI_OK;
}

int mdci_decode_device(mdci_decoder* d, const uint8_t* d_slots, int64_t slot_bytes, const int32_t* d_sizes, int skip_head, int skip_tail, int n, uint8_t* d_frames,
                       int64_t frame_stride, int32_t* d_status, void* stream) {
  const char* who = "mdci_decode_device";
  if (!d) return fail(MDCI_ERR_ARG, "%s: decoder is null", who);
  if (n < 0 || n > d->max_images) return fail(MDCI_ERR_ARG, "%s: %d frames, the decoder was made for 0..%d", who, n, d->max_images);
  if (n == 0) return MDCI_OK;
  if (!d_slots || !d_sizes || !d_frames || !d_status) return fail(MDCI_ERR_ARG, "%s: null device pointer", who);
  if ((uintptr_t)d_sizes % 4 || (uintptr_t)d_status % 4) return fail(MDCI_ERR_ARG, "%s: d_sizes and d_status are arrays of int32_t: 4-byte aligned", who);
  if (slot_bytes < 0) return fail(MDCI_ERR_ARG, "%s: slot_bytes %lld is negative", who, (long long)slot_bytes);
  if (skip_head < 0 || skip_tail < 0) return fail(MDCI_ERR_ARG, "%s: skip_head %d, skip_tail %d: neither may be negative", who, skip_head, skip_tail);
  if (frame_stride < (int64_t)d->w * d->h) return fail(MDCI_ERR_ARG, "%s: frame_stride %lld is below %d x %d", who, (long long)frame_stride, d->w, d->h);
  DeviceGuard dg(d->device);
  hipStream_t s = (hipStream_t)stream;
  const Input in = {d_slots, (long long)slot_bytes, d_sizes, skip_head, skip_tail};
  const long long N = n;
  const bool prof = d->profile;
  if (prof) (void)hipEventRecord(d->ev[0], s);
  pngd_front_kernel<<<grid_for(N), kFrontThreads, 0, s>>>(in, N, (uint32_t)d->F, d->d_filt, d->filt_stride, d->d_meta);
  if (prof) (void)hipEventRecord(d->ev[1], s);
  pngd_general_kernel<<<grid_for(N), 64, 0, s>>>(in, N, (uint32_t)d->F, d->d_filt, d->filt_stride, d->d_meta);
  if (prof) (void)hipEventRecord(d->ev[2], s);
  pngd_check_kernel<<<grid_for(N), 256, 0, s>>>(in, N, d->w, d->h, d->d_filt, d->filt_stride, d->d_meta);
  if (prof) (void)hipEventRecord(d->ev[3], s);
  pngd_unfilter_kernel<<<grid_for(N), 64, 0, s>>>(N, d->w, d->h, d->d_filt, d->filt_stride, d->d_meta, d_frames, (long long)frame_stride, d_status);
  if (prof) (void)hipEventRecord(d->ev[4], s), d->timed = true;
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(MDCI_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(err));
  return MDCI_OK;
}

int mdci_profile(mdci_decoder* d, int on) {
  if (!d) return fail(MDCI_ERR_ARG, "mdci_profile: decoder is null");
  DeviceGuard dg(d->device);
  for (hipEvent_t& e : d->ev)
    if (on && !e && hipEventCreate(&e) != hipSuccess) {
      e = nullptr;
      d->profile = false;
      return fail(MDCI_ERR_HIP, "mdci_profile: no event: %s", hipGetErrorString(hipGetLastError()));
    }
  d->profile = on != 0;
  d->timed = false;
  return MDCI_OK;
}

int mdci_kernel_ms(mdci_decoder* d, float ms[4]) {
  if (!d || !ms) return fail(MDCI_ERR_ARG, "mdci_kernel_ms: null argument");
  if (!d->timed) return fail(MDCI_ERR_ARG, "mdci_kernel_ms: no call has been timed (mdci_profile, then mdci_decode_device)");
  DeviceGuard dg(d->device);
  if (hipEventSynchronize(d->ev[4]) != hipSuccess) return fail(MDCI_ERR_HIP, "mdci_kernel_ms: %s", hipGetErrorString(hipGetLastError()));
  for (int k = 0; k < 4; k++)
    if (hipEventElapsedTime(&ms[k], d->ev[k], d->ev[k + 1]) != hipSuccess) return fail(MDCI_ERR_HIP, "mdci_kernel_ms: %s", hipGetErrorString(hipGetLastError()));
  return MDCI_OK;
}

void* mdci_stream(mdci_decoder* d) {
  if (!d) return nullptr;
  if (!d->stream) {
    DeviceGuard dg(d->device);
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) d->stream = nullptr;
  }
  return d->stream;
}

int mdci_synchronize(mdci_decoder* d) {
  if (!d) return fail(MDCI_ERR_ARG, "mdci_synchronize: decoder is null");
  if (!d->stream) return MDCI_OK;
  DeviceGuard dg(d->device);
  const hipError_t err = hipStreamSynchronize(d->stream);
  if (err != hipSuccess) return fail(MDCI_ERR_HIP, "mdci_synchronize: %s", hipGetErrorString(err));
  return MDCI_OK;
}

int mdci_decode_host(mdci_decoder* d, const void* const* streams, const int64_t* bytes, int n, int* status, const uint8_t** d_frames) {
  const char* who = "mdci_decode_host";
  if (!d) return fail(MDCI_ERR_ARG, "%s: decoder is null", who);
  if (n < 0 || n > d->max_images) return fail(MDCI_ERR_ARG, "%s: %d frames, the decoder was made for 0..%d", who, n, d->max_images);
  if (!d_frames) return fail(MDCI_ERR_ARG, "%s: d_frames is null", who);
  *d_frames = d->d_out;
  if (n == 0) return MDCI_OK;
  if (!streams || !bytes || !status) return fail(MDCI_ERR_ARG, "%s: null pointer", who);
  int64_t longest = 0;
  for (int f = 0; f < n; f++) {
    if (bytes[f] < 0 || bytes[f] > INT32_MAX || (bytes[f] > 0 && !streams[f])) return fail(MDCI_ERR_ARG, "%s: stream %d: %lld bytes at %p", who, f, (long long)bytes[f], streams[f]);
    if (bytes[f] > longest) longest = bytes[f];
  }
  DeviceGuard dg(d->device);
  const size_t head = ((size_t)n * 4 + 15) / 16 * 16, slot = ((size_t)longest + 15) / 16 * 16, need = head + slot * (size_t)n;
  if (!mdci_stream(d)) return fail(MDCI_ERR_HIP, "%s: no stream: %s", who, hipGetErrorString(hipGetLastError()));
  if (!d->d_out && (hipMalloc((void**)&d->d_out, (size_t)d->max_images * d->w * d->h) != hipSuccess ||
                    hipMalloc((void**)&d->d_status, (size_t)d->max_images * 4) != hipSuccess)) {
    (void)hipGetLastError();
    (void)hipFree(d->d_out);
    d->d_out = nullptr;
    return fail(MDCI_ERR_NOMEM, "%s: could not allocate %d frames of %d x %d", who, d->max_images, d->w, d->h);
  }
  if (need > d->stage_bytes) {
    (void)hipStreamSynchronize(d->stream);
    if (d->h_stage) (void)hipHostFree(d->h_stage);
    (void)hipFree(d->d_stage);
    d->h_stage = d->d_stage = nullptr;
    d->stage_bytes = 0;
    const size_t want = need + need / 4;  // some room: the next batch's longest stream is rarely the same
    if (hipHostMalloc((void**)&d->h_stage, want, hipHostMallocDefault) != hipSuccess || hipMalloc((void**)&d->d_stage, want) != hipSuccess) {
      (void)hipGetLastError();
      if (d->h_stage) (void)hipHostFree(d->h_stage);
      d->h_stage = nullptr;
      return fail(MDCI_ERR_NOMEM, "%s: could not allocate %zu bytes of staging", who, want);
    }
    d->stage_bytes = want;
  }
  int32_t* sizes = (int32_t*)d->h_stage;
  for (int f = 0; f < n; f++) {
    sizes[f] = (int32_t)bytes[f];
    if (bytes[f]) memcpy(d->h_stage + head + slot * (size_t)f, streams[f], (size_t)bytes[f]);
  }
  *d_frames = d->d_out;
  if (hipMemcpyAsync(d->d_stage, d->h_stage, need, hipMemcpyHostToDevice, d->stream) != hipSuccess)
    return fail(MDCI_ERR_HIP, "%s: upload failed: %s", who, hipGetErrorString(hipGetLastError()));
  const int rc = mdci_decode_device(d, d->d_stage + head, (int64_t)slot, (const int32_t*)d->d_stage, 0, 0, n, d->d_out, (int64_t)d->w * d->h, d->d_status, d->stream);
  if (rc != MDCI_OK) return rc;
  if (hipMemcpyAsync(status, d->d_status, (size_t)n * 4, hipMemcpyDeviceToHost, d->stream) != hipSuccess || hipStreamSynchronize(d->stream) != hipSuccess)
    return fail(MDCI_ERR_HIP, "%s: the decode failed: %s", who, hipGetErrorString(hipGetLastError()));
  return MDCI_OK;
}

}  // extern "C"
