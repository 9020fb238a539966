// libmdc_pngdx.so (include/mdc_pngdx.h): PNG frames decoded on the device, ordinary DEFLATE streams in parallel.  One translation
// unit; it shares png_decode_kernels.h (the four kernels of libmdc_pngd.so and the host helpers) with mdc_pngd.hip, and
// png_tokens_core.h (the token path, phase by phase) with the CPU test program.  It links no library of this project.
//
// One call is six kernels, with no host round trip between them:
//   pngd_front_kernel     as in libmdc_pngd.so: classifies; decodes the literal-only and the stored-only streams
//   pngdx_tokens_kernel   one workgroup of 1024 threads per image that is not done yet: pngx::decode_image -- whole tokens from guessed
//                         entries that relax to the sequential decoder's, a scan for the output positions, literals and per-byte
//                         source indices written, the indices resolved by pointer doubling, one gather.  Gives up on whatever is
//                         not a valid stream of F bytes and leaves that frame as it found it.
//   pngd_general_kernel   the sequential decoder for what is left: it names the reason
//   pngd_check_kernel     Adler-32, trailer, filter types
//   pngdx_settle_kernel   a frame of the token path that the checks refused is reported with the general path (mdc_pngdx.h)
//   pngd_unfilter_kernel  pixels and d_status
#include "../../include/mdc_pngdx.h"

#include <new>

#include "png_decode_kernels.h"
#include "png_tokens_core.h"

static_assert(MDCX_ST_TRUNCATED == pngd::ST_TRUNCATED && MDCX_ST_ZLIB_HEADER == pngd::ST_ZLIB_HEADER && MDCX_ST_BLOCK_TYPE == pngd::ST_BLOCK_TYPE &&
                  MDCX_ST_STORED_LEN == pngd::ST_STORED_LEN && MDCX_ST_BAD_CODE == pngd::ST_BAD_CODE && MDCX_ST_UNDEFINED_SYMBOL == pngd::ST_UNDEFINED_SYMBOL &&
                  MDCX_ST_DISTANCE == pngd::ST_DISTANCE && MDCX_ST_OUTPUT_SIZE == pngd::ST_OUTPUT_SIZE && MDCX_ST_FILTER_TYPE == pngd::ST_FILTER_TYPE &&
                  MDCX_ST_ADLER == pngd::ST_ADLER && MDCX_PATH_PARALLEL == pngd::PATH_PARALLEL && MDCX_PATH_STORED == pngd::PATH_STORED &&
                  MDCX_PATH_GENERAL == pngd::PATH_GENERAL && MDCX_PATH_TOKENS == pngx::PATH_TOKENS && MDCX_MAX_STORED_BLOCKS == pngd::kMaxStoredBlocks,
              "include/mdc_pngdx.h, png_inflate_core.h and png_tokens_core.h name the same codes");
static_assert(pngx::kThreads == 1024 && pngx::kSubBits >= 48, "a token fits a subsequence; the workgroup is the largest there is");

namespace {

// The workgroup as pngx::decode_image's team.  __syncthreads() orders the LDS arrays and, with the workgroup-scope fence, the filtered
// bytes and source indices that one wave stores and another loads: all of them go through this compute unit's vector cache (as
// WaveOut::copy in png_decode_kernels.h documents it).
struct WorkgroupTeam {
  template <class Fn>
  __device__ __forceinline__ void each(Fn fn) const {
    fn((int)threadIdx.x);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();
  }
  template <class Fn>
  __device__ __forceinline__ bool each_or(Fn fn) const {
    const bool v = fn((int)threadIdx.x);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    return __syncthreads_or(v ? 1 : 0) != 0;
  }
};

__global__ __launch_bounds__(pngx::kThreads) void pngdx_tokens_kernel(Input in, long long nimages, uint32_t F, uint8_t* __restrict__ filt, long long filt_stride,
                                                                      uint32_t* __restrict__ src, uint32_t* __restrict__ meta) {
  __shared__ pngx::Shared S;
  const WorkgroupTeam team;
  for (long long f = blockIdx.x; f < nimages; f += gridDim.x) {
    __syncthreads();  // nobody still reads S for the previous image
    if (meta[f * kMetaWords + 3] != 0) continue;  // done by the front kernel (the same for the whole workgroup)
    pngx::Image im;
    im.p = stream_of(in, f, &im.n);
    im.F = F, im.out = filt + f * filt_stride, im.src = src + f * filt_stride;
    uint32_t end_byte = 0;
    const bool ok = pngx::decode_image(team, S, im, &end_byte);
    if (ok && threadIdx.x == 0) {
      meta[f * kMetaWords + 0] = 0, meta[f * kMetaWords + 1] = pngx::PATH_TOKENS;
      meta[f * kMetaWords + 2] = end_byte, meta[f * kMetaWords + 3] = 1;
    }
  }
}

__global__ __launch_bounds__(256) void pngdx_settle_kernel(long long nimages, uint32_t* __restrict__ meta) {
  for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < nimages; f += (long long)gridDim.x * 256)
    if (meta[f * kMetaWords + 0] != 0 && meta[f * kMetaWords + 1] == (uint32_t)pngx::PATH_TOKENS) meta[f * kMetaWords + 1] = pngd::PATH_GENERAL;
}

}  // namespace

struct mdcx_decoder {
  int device = -1, w = 0, h = 0, max_images = 0;
  long long F = 0, filt_stride = 0;
  uint8_t* d_filt = nullptr;
  uint32_t* d_src = nullptr;  // the token path's source index of every filtered byte
  uint32_t* d_meta = nullptr;
  // mdcx_decode_host: made at its first call
  hipStream_t stream = nullptr;
  uint8_t* h_stage = nullptr;  // pinned: n sizes (padded to 16 bytes), then n slots
  uint8_t* d_stage = nullptr;
  size_t stage_bytes = 0;
  uint8_t* d_out = nullptr;
  int32_t* d_status = nullptr;
  // mdcx_profile: events around the kernels of a call
  bool profile = false, timed = false;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};

extern "C" {

const char* mdcx_last_error(void) { return g_error; }

int64_t mdcx_scratch_bytes(int w, int h, int max_images) {
  if (w < 1 || h < 1 || max_images < 1) return -1;
  if ((1ll + w) > (1ll << 28) / h) return -1;
  const long long per_image = 5 * filt_stride_of(w, h) + 4 * kMetaWords;
  if (per_image > (1ll << 40) / max_images) return -1;
  return per_image * max_images;
}

void mdcx_destroy(mdcx_decoder* d) {
  if (!d) return;
  {
    DeviceGuard dg(d->device);
    if (d->stream) (void)hipStreamSynchronize(d->stream);
    (void)hipFree(d->d_filt);
    (void)hipFree(d->d_src);
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

int mdcx_create(int device, int w, int h, int max_images, mdcx_decoder** out) {
  if (!out) return fail(MDCX_ERR_ARG, "mdcx_create: out is null");
  *out = nullptr;
  if (max_images < 1) return fail(MDCX_ERR_ARG, "mdcx_create: max_images %d is below 1", max_images);
  if (w < 1 || h < 1) return fail(MDCX_ERR_SIZE, "mdcx_create: %d x %d: width and height start at 1", w, h);
  if ((1ll + w) > (1ll << 28) / h) return fail(MDCX_ERR_SIZE, "mdcx_create: a %d x %d image has more than 2^28 filtered bytes", w, h);
  const int64_t scratch = mdcx_scratch_bytes(w, h, max_images);
  if (scratch < 0) return fail(MDCX_ERR_SIZE, "mdcx_create: %d images of %d x %d: the scratch passes 2^40 bytes", max_images, w, h);
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return fail(MDCX_ERR_NO_DEVICE, "mdcx_create: no HIP device");
  if (device >= count) return fail(MDCX_ERR_NO_DEVICE, "mdcx_create: device %d of %d", device, count);
  if (device < 0 && hipGetDevice(&device) != hipSuccess) return fail(MDCX_ERR_HIP, "mdcx_create: hipGetDevice failed");
  DeviceGuard dg(device);
  mdcx_decoder* d = new (std::nothrow) mdcx_decoder;
  if (!d) return fail(MDCX_ERR_NOMEM, "mdcx_create: out of host memory");
  d->device = device, d->w = w, d->h = h, d->max_images = max_images;
  d->F = (1ll + w) * h, d->filt_stride = filt_stride_of(w, h);
  if (hipMalloc((void**)&d->d_filt, (size_t)d->filt_stride * (size_t)max_images) != hipSuccess ||
      hipMalloc((void**)&d->d_src, (size_t)d->filt_stride * (size_t)max_images * 4) != hipSuccess ||
      hipMalloc((void**)&d->d_meta, (size_t)max_images * kMetaWords * 4) != hipSuccess) {
    (void)hipGetLastError();
    mdcx_destroy(d);
    return fail(MDCX_ERR_NOMEM, "mdcx_create: could not allocate the scratch arrays of %d images of %d x %d", max_images, w, h);
  }
  *out = d;
  return MDCX_OK;
}

int mdcx_decode_device(mdcx_decoder* d, const uint8_t* d_slots, int64_t slot_bytes, const int32_t* d_sizes, int skip_head, int skip_tail, int n, uint8_t* d_frames,
                       int64_t frame_stride, int32_t* d_status, void* stream) {
  const char* who = "mdcx_decode_device";
  if (!d) return fail(MDCX_ERR_ARG, "%s: decoder is null", who);
  if (n < 0 || n > d->max_images) return fail(MDCX_ERR_ARG, "%s: %d frames, the decoder was made for 0..%d", who, n, d->max_images);
  if (n == 0) return MDCX_OK;
  if (!d_slots || !d_sizes || !d_frames || !d_status) return fail(MDCX_ERR_ARG, "%s: null device pointer", who);
  if ((uintptr_t)d_sizes % 4 || (uintptr_t)d_status % 4) return fail(MDCX_ERR_ARG, "%s: d_sizes and d_status are arrays of int32_t: 4-byte aligned", who);
  if (slot_bytes < 0) return fail(MDCX_ERR_ARG, "%s: slot_bytes %lld is negative", who, (long long)slot_bytes);
  if (skip_head < 0 || skip_tail < 0) return fail(MDCX_ERR_ARG, "%s: skip_head %d, skip_tail %d: neither may be negative", who, skip_head, skip_tail);
  if (frame_stride < (int64_t)d->w * d->h) return fail(MDCX_ERR_ARG, "%s: frame_stride %lld is below %d x %d", who, (long long)frame_stride, d->w, d->h);
  DeviceGuard dg(d->device);
  hipStream_t s = (hipStream_t)stream;
  const Input in = {d_slots, (long long)slot_bytes, d_sizes, skip_head, skip_tail};
  const long long N = n;
  const bool prof = d->profile;
  if (prof) (void)hipEventRecord(d->ev[0], s);
  pngd_front_kernel<<<grid_for(N), kFrontThreads, 0, s>>>(in, N, (uint32_t)d->F, d->d_filt, d->filt_stride, d->d_meta);
  if (prof) (void)hipEventRecord(d->ev[1], s);
  pngdx_tokens_kernel<<<grid_for(N), pngx::kThreads, 0, s>>>(in, N, (uint32_t)d->F, d->d_filt, d->filt_stride, d->d_src, d->d_meta);
  if (prof) (void)hipEventRecord(d->ev[2], s);
  pngd_general_kernel<<<grid_for(N), 64, 0, s>>>(in, N, (uint32_t)d->F, d->d_filt, d->filt_stride, d->d_meta);
  if (prof) (void)hipEventRecord(d->ev[3], s);
  pngd_check_kernel<<<grid_for(N), 256, 0, s>>>(in, N, d->w, d->h, d->d_filt, d->filt_stride, d->d_meta);
  pngdx_settle_kernel<<<grid_for((N + 255) / 256), 256, 0, s>>>(N, d->d_meta);
  if (prof) (void)hipEventRecord(d->ev[4], s);
  pngd_unfilter_kernel<<<grid_for(N), 64, 0, s>>>(N, d->w, d->h, d->d_filt, d->filt_stride, d->d_meta, d_frames, (long long)frame_stride, d_status);
  if (prof) (void)hipEventRecord(d->ev[5], s), d->timed = true;
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(MDCX_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(err));
  return MDCX_OK;
}

int mdcx_profile(mdcx_decoder* d, int on) {
  if (!d) return fail(MDCX_ERR_ARG, "mdcx_profile: decoder is null");
  DeviceGuard dg(d->device);
  for (hipEvent_t& e : d->ev)
    if (on && !e && hipEventCreate(&e) != hipSuccess) {
      e = nullptr;
      d->profile = false;
      return fail(MDCX_ERR_HIP, "mdcx_profile: no event: %s", hipGetErrorString(hipGetLastError()));
    }
  d->profile = on != 0;
  d->timed = false;
  return MDCX_OK;
}

int mdcx_kernel_ms(mdcx_decoder* d, float ms[5]) {
  if (!d || !ms) return fail(MDCX_ERR_ARG, "mdcx_kernel_ms: null argument");
  if (!d->timed) return fail(MDCX_ERR_ARG, "mdcx_kernel_ms: no call has been timed (mdcx_profile, then mdcx_decode_device)");
  DeviceGuard dg(d->device);
  if (hipEventSynchronize(d->ev[5]) != hipSuccess) return fail(MDCX_ERR_HIP, "mdcx_kernel_ms: %s", hipGetErrorString(hipGetLastError()));
  for (int k = 0; k < 5; k++)
    if (hipEventElapsedTime(&ms[k], d->ev[k], d->ev[k + 1]) != hipSuccess) return fail(MDCX_ERR_HIP, "mdcx_kernel_ms: %s", hipGetErrorString(hipGetLastError()));
  return MDCX_OK;
}

void* mdcx_stream(mdcx_decoder* d) {
  if (!d) return nullptr;
  if (!d->stream) {
    DeviceGuard dg(d->device);
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) d->stream = nullptr;
  }
  return d->stream;
}

int mdcx_synchronize(mdcx_decoder* d) {
  if (!d) return fail(MDCX_ERR_ARG, "mdcx_synchronize: decoder is null");
  if (!d->stream) return MDCX_OK;
  DeviceGuard dg(d->device);
  const hipError_t err = hipStreamSynchronize(d->stream);
  if (err != hipSuccess) return fail(MDCX_ERR_HIP, "mdcx_synchronize: %s", hipGetErrorString(err));
  return MDCX_OK;
}

int mdcx_decode_host(mdcx_decoder* d, const void* const* streams, const int64_t* bytes, int n, int* status, const uint8_t** d_frames) {
  const char* who = "mdcx_decode_host";
  if (!d) return fail(MDCX_ERR_ARG, "%s: decoder is null", who);
  if (n < 0 || n > d->max_images) return fail(MDCX_ERR_ARG, "%s: %d frames, the decoder was made for 0..%d", who, n, d->max_images);
  if (!d_frames) return fail(MDCX_ERR_ARG, "%s: d_frames is null", who);
  *d_frames = d->d_out;
  if (n == 0) return MDCX_OK;
  if (!streams || !bytes || !status) return fail(MDCX_ERR_ARG, "%s: null pointer", who);
  int64_t longest = 0;
  for (int f = 0; f < n; f++) {
    if (bytes[f] < 0 || bytes[f] > INT32_MAX || (bytes[f] > 0 && !streams[f])) return fail(MDCX_ERR_ARG, "%s: stream %d: %lld bytes at %p", who, f, (long long)bytes[f], streams[f]);
    if (bytes[f] > longest) longest = bytes[f];
  }
  DeviceGuard dg(d->device);
  const size_t head = ((size_t)n * 4 + 15) / 16 * 16, slot = ((size_t)longest + 15) / 16 * 16, need = head + slot * (size_t)n;
  if (!mdcx_stream(d)) return fail(MDCX_ERR_HIP, "%s: no stream: %s", who, hipGetErrorString(hipGetLastError()));
  if (!d->d_out && (hipMalloc((void**)&d->d_out, (size_t)d->max_images * d->w * d->h) != hipSuccess ||
                    hipMalloc((void**)&d->d_status, (size_t)d->max_images * 4) != hipSuccess)) {
    (void)hipGetLastError();
    (void)hipFree(d->d_out);
    d->d_out = nullptr;
    return fail(MDCX_ERR_NOMEM, "%s: could not allocate %d frames of %d x %d", who, d->max_images, d->w, d->h);
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
      return fail(MDCX_ERR_NOMEM, "%s: could not allocate %zu bytes of staging", who, want);
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
    return fail(MDCX_ERR_HIP, "%s: upload failed: %s", who, hipGetErrorString(hipGetLastError()));
  const int rc = mdcx_decode_device(d, d->d_stage + head, (int64_t)slot, (const int32_t*)d->d_stage, 0, 0, n, d->d_out, (int64_t)d->w * d->h, d->d_status, d->stream);
  if (rc != MDCX_OK) return rc;
  if (hipMemcpyAsync(status, d->d_status, (size_t)n * 4, hipMemcpyDeviceToHost, d->stream) != hipSuccess || hipStreamSynchronize(d->stream) != hipSuccess)
    return fail(MDCX_ERR_HIP, "%s: the decode failed: %s", who, hipGetErrorString(hipGetLastError()));
  return MDCX_OK;
}

}  // extern "C"
