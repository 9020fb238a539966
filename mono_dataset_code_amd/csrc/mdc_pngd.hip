// libmdc_pngd.so (include/mdc_pngd.h): PNG frames decoded on the device.  One translation unit; it shares png_inflate_core.h with
// the CPU test program, and its kernels and host side (png_decode_kernels.h) with mdc_pngdx.hip, which is a library of its own.
//
// One call is the four kernels of png_decode_kernels.h, with no host round trip between them: front, general, check, unfilter.
#include "../../include/mdc_pngd.h"

#include "png_decode_kernels.h"

static_assert(MDCI_ST_TRUNCATED == pngd::ST_TRUNCATED && MDCI_ST_ZLIB_HEADER == pngd::ST_ZLIB_HEADER && MDCI_ST_BLOCK_TYPE == pngd::ST_BLOCK_TYPE &&
                  MDCI_ST_STORED_LEN == pngd::ST_STORED_LEN && MDCI_ST_BAD_CODE == pngd::ST_BAD_CODE && MDCI_ST_UNDEFINED_SYMBOL == pngd::ST_UNDEFINED_SYMBOL &&
                  MDCI_ST_DISTANCE == pngd::ST_DISTANCE && MDCI_ST_OUTPUT_SIZE == pngd::ST_OUTPUT_SIZE && MDCI_ST_FILTER_TYPE == pngd::ST_FILTER_TYPE &&
                  MDCI_ST_ADLER == pngd::ST_ADLER && MDCI_PATH_PARALLEL == pngd::PATH_PARALLEL && MDCI_PATH_STORED == pngd::PATH_STORED &&
                  MDCI_PATH_GENERAL == pngd::PATH_GENERAL && MDCI_MAX_STORED_BLOCKS == pngd::kMaxStoredBlocks,
              "include/mdc_pngd.h and png_inflate_core.h name the same codes");

static_assert(MDCI_OK == kOk && MDCI_ERR_ARG == kErrArg && MDCI_ERR_SIZE == kErrSize && MDCI_ERR_HIP == kErrHip && MDCI_ERR_NO_DEVICE == kErrNoDevice &&
                  MDCI_ERR_NOMEM == kErrNoMem,
              "include/mdc_pngd.h and codec_host.h name the same codes");

struct mdci_decoder : Decoder {
  void** extra() { return nullptr; }
};

namespace {

constexpr Params kParams = {"mdci", 0, 4};

// the kernels of one call (png_decode_kernels.h: decode_device)
struct Launch {
  template <class Mark>
  void operator()(mdci_decoder* d, const Call& c, const Mark& mark) const {
    mark();
    pngd_front_kernel<<<grid_for(c.N), kFrontThreads, 0, c.s>>>(c.in, c.N, (uint32_t)d->F, d->d_filt, d->filt_stride, d->d_meta);
    mark();
    pngd_general_kernel<<<grid_for(c.N), 64, 0, c.s>>>(c.in, c.N, (uint32_t)d->F, d->d_filt, d->filt_stride, d->d_meta);
    mark();
    pngd_check_kernel<<<grid_for(c.N), 256, 0, c.s>>>(c.in, c.N, d->w, d->h, d->d_filt, d->filt_stride, d->d_meta);
    mark();
    pngd_unfilter_kernel<<<grid_for(c.N), 64, 0, c.s>>>(c.N, d->w, d->h, d->d_filt, d->filt_stride, d->d_meta, c.frames, c.frame_stride, c.status);
    mark();
  }
};

}  // namespace

extern "C" {

const char* mdci_last_error(void) { return g_error; }

int64_t mdci_scratch_bytes(int w, int h, int max_images) { return scratch_bytes(kParams, w, h, max_images); }

void mdci_destroy(mdci_decoder* d) { destroy(d); }

int mdci_create(int device, int w, int h, int max_images, mdci_decoder** out) { return create("mdci_create", kParams, device, w, h, max_images, out); }

int mdci_decode_device(mdci_decoder* d, const uint8_t* d_slots, int64_t slot_bytes, const int32_t* d_sizes, int skip_head, int skip_tail, int n, uint8_t* d_frames,
                       int64_t frame_stride, int32_t* d_status, void* stream) {
  return decode_device(kParams, d, d_slots, slot_bytes, d_sizes, skip_head, skip_tail, n, d_frames, frame_stride, d_status, stream, Launch());
}

int mdci_profile(mdci_decoder* d, int on) { return profile(kParams, d, on); }

int mdci_kernel_ms(mdci_decoder* d, float ms[4]) { return kernel_ms(kParams, d, ms); }

void* mdci_stream(mdci_decoder* d) { return own_stream(d); }

int mdci_synchronize(mdci_decoder* d) { return synchronize(kParams, d); }

int mdci_decode_host(mdci_decoder* d, const void* const* streams, const int64_t* bytes, int n, int* status, const uint8_t** d_frames) {
  return decode_host(kParams, d, streams, bytes, n, status, d_frames, Launch());
}

}  // extern "C"
