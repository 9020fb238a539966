// libmdc_jenc.so -- baseline JPEG encoder for device-resident grayscale frames (include/mdc_jenc.h), gfx950.
// A library of its own: no mdc_ctx, nothing of libmdc_hip.so; functions take a device and a stream.
//
// One call encodes a batch of frames in five launches, all integer, all deterministic (a sixth kernel, jenc_gather_kernel, serves
// mdcj_fetch: the files back to back, so that one copy brings them to the host):
//   jenc_fdct_quant_kernel  pixels -> quantised coefficients, zigzag order, int16 (8 threads per 8x8 block, through LDS)
//   jenc_count_kernel       one thread per block: the number of bits its Huffman code takes
//   jenc_scan_kernel        one workgroup per frame: exclusive scan of the bit counts -> each block's bit offset; zeroes the
//                           frame's part of the bit stream that will be written
//   jenc_pack_kernel        one thread per block: its code words at its bit offset (integer atomicOr where a 32-bit word is
//                           shared with a neighbour block, plain stores inside)
//   jenc_stuff_kernel       one workgroup per frame: header, the stream's bytes with 0x00 after every 0xFF (a scan over
//                           bytes), the 1-bit padding of the last byte, EOI, and the length
// The DC difference needs only the previous block's coefficient, which the first kernel has written, so blocks are independent.
// No kernel keeps a runtime-indexed per-thread array: coefficients live in registers with static indices or in LDS.
#include "../../include/mdc_jenc.h"
#include "jpeg_encode_core.h"

namespace {

constexpr Params kParams = {"mdcj", 416, 20 + 63 * 26};  // include/mdc_jenc.h: the bound's derivation

// one thread per block of the batch; total = frames * nblocks < 2^31
__global__ __launch_bounds__(256) void jenc_count_kernel(const int16_t* __restrict__ coef, int nblocks, int total, const DeviceTables* __restrict__ tab,
                                                         uint32_t* __restrict__ bits) {
  __shared__ uint32_t s_ac[256], s_dc[16];
  load_tables(tab, s_ac, s_dc);
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int prev_dc = (i % nblocks) ? coef[(i - 1) * 64] : 0;
  BitCounter count;
  walk_block(coef + i * 64, prev_dc, s_ac, s_dc, count);
  bits[i] = count.bits;
}

__global__ __launch_bounds__(256) void jenc_pack_kernel(const int16_t* __restrict__ coef, int nblocks, int total, const DeviceTables* __restrict__ tab,
                                                        const uint32_t* __restrict__ bit_offset, uint32_t* __restrict__ stream, long long stream_words) {
  __shared__ uint32_t s_ac[256], s_dc[16];
  load_tables(tab, s_ac, s_dc);
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int prev_dc = (i % nblocks) ? coef[(i - 1) * 64] : 0;
  BitPacker pack(stream + (i / nblocks) * stream_words, bit_offset[i]);
  walk_block(coef + i * 64, prev_dc, s_ac, s_dc, pack);
  pack.finish();
}

// one workgroup of 1024 per frame.  Per iteration 16 stream bytes per thread: count the 0xFF among them, scan, lay the stuffed
// bytes out in LDS, copy them out with consecutive threads on consecutive bytes.
__global__ __launch_bounds__(1024) void jenc_stuff_kernel(const uint32_t* __restrict__ stream, long long stream_words, const uint32_t* __restrict__ frame_bits,
                                                          const DeviceTables* __restrict__ tab, uint8_t* __restrict__ out, long long slot_bytes,
                                                          int32_t* __restrict__ sizes) {
  __shared__ uint8_t staged[2 * kStuffChunk];
  __shared__ uint32_t scratch[16];
  const int t = threadIdx.x;
  const uint32_t* __restrict__ s = stream + (long long)blockIdx.x * stream_words;
  uint8_t* __restrict__ o = out + (long long)blockIdx.x * slot_bytes;
  const uint32_t nbits = frame_bits[blockIdx.x];
  const uint32_t nbytes = (nbits + 7u) >> 3;
  const uint32_t pad = (nbits & 7u) ? (0xffu >> (nbits & 7u)) : 0u;  // 1-bits that fill the last byte
  for (int k = t; k < kHeaderBytes; k += 1024) o[k] = tab->header[k];
  uint32_t pos = kHeaderBytes;
  for (uint32_t base = 0; base < nbytes; base += kStuffChunk) {
    const uint32_t byte0 = base + (uint32_t)t * 16u;
    uint32_t wd[4];
    uint32_t ff = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t at = byte0 + 4u * j;  // a multiple of 4
      uint32_t x = at < nbytes ? s[at >> 2] : 0u;
      if (pad && at == ((nbytes - 1u) & ~3u)) x |= pad << (24u - 8u * ((nbytes - 1u) & 3u));
      wd[j] = x;
#pragma unroll
      for (int q = 0; q < 4; q++) ff += (at + q < nbytes && ((x >> (24 - 8 * q)) & 0xffu) == 0xffu) ? 1u : 0u;
    }
    const uint32_t mine = (byte0 < nbytes ? min(16u, nbytes - byte0) : 0u) + ff;
    uint32_t all;
    uint32_t lp = workgroup_scan_1024(mine, scratch, &all) - mine;
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t v = (wd[j] >> (24 - 8 * q)) & 0xffu;
        if (byte0 + 4u * j + q < nbytes) {
          staged[lp++] = (uint8_t)v;
          if (v == 0xffu) staged[lp++] = 0;
        }
      }
    }
    __syncthreads();
    for (uint32_t k = t; k < all; k += 1024) o[pos + k] = staged[k];
    pos += all;
    __syncthreads();  // staged is rewritten by the next iteration
  }
  if (t == 0) {
    o[pos] = 0xff;
    o[pos + 1] = 0xd9;
    sizes[blockIdx.x] = (int32_t)(pos + 2);
  }
}

}  // namespace

static_assert(MDCJ_OK == kOk && MDCJ_ERR_ARG == kErrArg && MDCJ_ERR_SIZE == kErrSize && MDCJ_ERR_HIP == kErrHip && MDCJ_ERR_NO_DEVICE == kErrNoDevice &&
                  MDCJ_ERR_NOMEM == kErrNoMem,
              "include/mdc_jenc.h and codec_host.h name the same codes");

struct mdcj_encoder : Encoder {
  bool alloc_extra() { return true; }
  void free_extra() {}
};

namespace {

template <typename T>
int encode(const char* who, mdcj_encoder* e, const T* d_frames, int64_t frame_stride, int nframes, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
           void* stream) {
  bool go;
  if (int rc = check_encode(who, kParams, e, d_frames, frame_stride, nframes, d_out, slot_bytes, d_sizes, &go); rc || !go) return rc;
  DeviceGuard dg(e->device);
  hipStream_t s = (hipStream_t)stream;
  const int nblocks = e->nblocks, bw = (e->w + 7) / 8;
  const int total = nblocks * nframes;  // < 2^31: mdcj_create
  const unsigned groups = (unsigned)((nblocks + kGroupBlocks - 1) / kGroupBlocks);
  const uint16_t* d_qdiv = reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(e->d_tab) + offsetof(DeviceTables, qdiv));
  for (int f0 = 0; f0 < nframes; f0 += 65535) {  // a grid's y dimension is 16-bit
    const unsigned nf = (unsigned)(nframes - f0 < 65535 ? nframes - f0 : 65535);
    jenc_fdct_quant_kernel<T><<<dim3(groups, nf), 256, 0, s>>>(d_frames, (long long)frame_stride, f0, e->w, e->h, bw, nblocks, d_qdiv, e->d_coef);
  }
  const unsigned per_block_grid = (unsigned)(((long long)total + 255) / 256);
  jenc_count_kernel<<<per_block_grid, 256, 0, s>>>(e->d_coef, nblocks, total, e->d_tab, e->d_bits);
  jenc_scan_kernel<<<(unsigned)nframes, 1024, 0, s>>>(e->d_bits, nblocks, e->d_frame_bits, e->d_stream, e->stream_words);
  jenc_pack_kernel<<<per_block_grid, 256, 0, s>>>(e->d_coef, nblocks, total, e->d_tab, e->d_bits, e->d_stream, e->stream_words);
  jenc_stuff_kernel<<<(unsigned)nframes, 1024, 0, s>>>(e->d_stream, e->stream_words, e->d_frame_bits, e->d_tab, d_out, (long long)slot_bytes, d_sizes);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(MDCJ_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(err));
  return MDCJ_OK;
}

}  // namespace

extern "C" {

int64_t mdcj_jpeg_bound(int w, int h) { return jpeg_bound(kParams, w, h); }

const char* mdcj_last_error(void) { return g_error; }

void mdcj_destroy(mdcj_encoder* enc) { destroy(enc); }

int mdcj_create(int device, int w, int h, int quality, int max_frames, mdcj_encoder** out) {
  return create("mdcj_create", kParams, device, w, h, quality, max_frames, out);
}

int mdcj_encode_f32_device(mdcj_encoder* enc, const float* d_frames, int64_t frame_stride, int nframes, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
                           void* stream) {
  return encode("mdcj_encode_f32_device", enc, d_frames, frame_stride, nframes, d_out, slot_bytes, d_sizes, stream);
}

int mdcj_encode_u8_device(mdcj_encoder* enc, const uint8_t* d_frames, int64_t frame_stride, int nframes, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
                          void* stream) {
  return encode("mdcj_encode_u8_device", enc, d_frames, frame_stride, nframes, d_out, slot_bytes, d_sizes, stream);
}

int mdcj_output_device(mdcj_encoder* enc, uint8_t** d_out, int64_t* slot_bytes, int32_t** d_sizes) { return output_device(kParams, enc, d_out, slot_bytes, d_sizes); }

int64_t mdcj_fetch(mdcj_encoder* enc, const uint8_t* d_out, int64_t slot_bytes, const int32_t* d_sizes, int nframes, uint8_t* h_out, int64_t h_capacity,
                   int32_t* h_sizes, void* stream) {
  return fetch(kParams, enc, d_out, slot_bytes, d_sizes, nframes, h_out, h_capacity, h_sizes, stream);
}

}  // extern "C"
