// libmdc_pngdx.so (include/mdc_pngdx.h): PNG frames decoded on the device, ordinary DEFLATE streams in parallel.  One translation
// unit; it shares png_decode_kernels.h (the four kernels of libmdc_pngd.so and the host side) with mdc_pngd.hip, and
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

#include "png_decode_kernels.h"
#include "png_tokens_core.h"

static_assert(MDCX_ST_TRUNCATED == pngd::ST_TRUNCATED && MDCX_ST_ZLIB_HEADER == pngd::ST_ZLIB_HEADER && MDCX_ST_BLOCK_TYPE == pngd::ST_BLOCK_TYPE &&
                  MDCX_ST_STORED_LEN == pngd::ST_STORED_LEN && MDCX_ST_BAD_CODE == pngd::ST_BAD_CODE && MDCX_ST_UNDEFINED_SYMBOL == pngd::ST_UNDEFINED_SYMBOL &&
                  MDCX_ST_DISTANCE == pngd::ST_DISTANCE && MDCX_ST_OUTPUT_SIZE == pngd::ST_OUTPUT_SIZE && MDCX_ST_FILTER_TYPE == pngd::ST_FILTER_TYPE &&
                  MDCX_ST_ADLER == pngd::ST_ADLER && MDCX_PATH_PARALLEL == pngd::PATH_PARALLEL && MDCX_PATH_STORED == pngd::PATH_STORED &&
                  MDCX_PATH_GENERAL == pngd::PATH_GENERAL && MDCX_PATH_TOKENS == pngx::PATH_TOKENS && MDCX_MAX_STORED_BLOCKS == pngd::kMaxStoredBlocks,
              "include/mdc_pngdx.h, png_inflate_core.h and png_tokens_core.h name the same codes");
static_assert(MDCX_OK == kOk && MDCX_ERR_ARG == kErrArg && MDCX_ERR_SIZE == kErrSize && MDCX_ERR_HIP == kErrHip && MDCX_ERR_NO_DEVICE == kErrNoDevice &&
                  MDCX_ERR_NOMEM == kErrNoMem,
              "include/mdc_pngdx.h and codec_host.h name the same codes (so MDCX_ERR_* equals MDCI_ERR_*, which mdc_pngd.hip holds to them too)");
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

struct mdcx_decoder : Decoder {
  uint32_t* d_src = nullptr;  // the token path's source index of every filtered byte
  void** extra() { return (void**)&d_src; }
};

namespace {

constexpr Params kParams = {"mdcx", 4, 5};

// the kernels of one call (png_decode_kernels.h: decode_device)
struct Launch {
  template <class Mark>
  void operator()(mdcx_decoder* d, const Call& c, const Mark& mark) const {
    mark();
    pngd_front_kernel<<<grid_for(c.N), kFrontThreads, 0, c.s>>>(c.in, c.N, (uint32_t)d->F, d->d_filt, d->filt_stride, d->d_meta);
    mark();
    pngdx_tokens_kernel<<<grid_for(c.N), pngx::kThreads, 0, c.s>>>(c.in, c.N, (uint32_t)d->F, d->d_filt, d->filt_stride, d->d_src, d->d_meta);
    mark();
    pngd_general_kernel<<<grid_for(c.N), 64, 0, c.s>>>(c.in, c.N, (uint32_t)d->F, d->d_filt, d->filt_stride, d->d_meta);
    mark();
    pngd_check_kernel<<<grid_for(c.N), 256, 0, c.s>>>(c.in, c.N, d->w, d->h, d->d_filt, d->filt_stride, d->d_meta);
    pngdx_settle_kernel<<<grid_for((c.N + 255) / 256), 256, 0, c.s>>>(c.N, d->d_meta);
    mark();
    pngd_unfilter_kernel<<<grid_for(c.N), 64, 0, c.s>>>(c.N, d->w, d->h, d->d_filt, d->filt_stride, d->d_meta, c.frames, c.frame_stride, c.status);
    mark();
  }
};

}  // namespace

extern "C" {

const char* mdcx_last_error(void) { return g_error; }

int64_t mdcx_scratch_bytes(int w, int h, int max_images) { return scratch_bytes(kParams, w, h, max_images); }

void mdcx_destroy(mdcx_decoder* d) { destroy(d); }

int mdcx_create(int device, int w, int h, int max_images, mdcx_decoder** out) { return create("mdcx_create", kParams, device, w, h, max_images, out); }

int mdcx_decode_device(mdcx_decoder* d, const uint8_t* d_slots, int64_t slot_bytes, const int32_t* d_sizes, int skip_head, int skip_tail, int n, uint8_t* d_frames,
                       int64_t frame_stride, int32_t* d_status, void* stream) {
  return decode_device(kParams, d, d_slots, slot_bytes, d_sizes, skip_head, skip_tail, n, d_frames, frame_stride, d_status, stream, Launch());
}

int mdcx_profile(mdcx_decoder* d, int on) { return profile(kParams, d, on); }

int mdcx_kernel_ms(mdcx_decoder* d, float ms[5]) { return kernel_ms(kParams, d, ms); }

void* mdcx_stream(mdcx_decoder* d) { return own_stream(d); }

int mdcx_synchronize(mdcx_decoder* d) { return synchronize(kParams, d); }

int mdcx_decode_host(mdcx_decoder* d, const void* const* streams, const int64_t* bytes, int n, int* status, const uint8_t** d_frames) {
  return decode_host(kParams, d, streams, bytes, n, status, d_frames, Launch());
}

}  // extern "C"
