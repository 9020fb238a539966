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

#include <new>

namespace {

constexpr int kBitsPerBlockMax = 20 + 63 * 26;  // include/mdc_jenc.h: the bound's derivation

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

struct mdcj_encoder {
  int device = -1, w = 0, h = 0, quality = 0, max_frames = 0;
  int nblocks = 0;
  long long stream_words = 0;  // per frame
  DeviceTables* d_tab = nullptr;
  int16_t* d_coef = nullptr;
  uint32_t* d_bits = nullptr;
  uint32_t* d_frame_bits = nullptr;
  uint32_t* d_stream = nullptr;
  uint8_t* d_out = nullptr;  // mdcj_output_device: allocated on demand
  int32_t* d_sizes = nullptr;
  uint8_t* d_packed = nullptr;  // mdcj_fetch: the files back to back (grown on demand) and their offsets
  long long packed_capacity = 0;
  long long* d_offsets = nullptr;
};

extern "C" {

int64_t mdcj_jpeg_bound(int w, int h) {
  if (w < 1 || h < 1 || w > 65535 || h > 65535) return -1;
  return 1024 + 416 * blocks_of(w, h);
}

const char* mdcj_last_error(void) { return g_error; }

void mdcj_destroy(mdcj_encoder* enc) {
  if (!enc) return;
  {
    DeviceGuard dg(enc->device);
    (void)hipFree(enc->d_tab);
    (void)hipFree(enc->d_coef);
    (void)hipFree(enc->d_bits);
    (void)hipFree(enc->d_frame_bits);
    (void)hipFree(enc->d_stream);
    (void)hipFree(enc->d_out);
    (void)hipFree(enc->d_sizes);
    (void)hipFree(enc->d_packed);
    (void)hipFree(enc->d_offsets);
  }
  delete enc;
}

int mdcj_create(int device, int w, int h, int quality, int max_frames, mdcj_encoder** out) {
  if (!out) return fail(MDCJ_ERR_ARG, "mdcj_create: out is null");
  *out = nullptr;
  if (w < 1 || h < 1 || w > 65535 || h > 65535) return fail(MDCJ_ERR_SIZE, "mdcj_create: %d x %d is outside 1..65535 (the SOF0 fields are 16-bit)", w, h);
  if (quality < 1 || quality > 100) return fail(MDCJ_ERR_ARG, "mdcj_create: quality %d is outside 1..100", quality);
  if (max_frames < 1) return fail(MDCJ_ERR_ARG, "mdcj_create: max_frames %d is below 1", max_frames);
  const long long nblocks = blocks_of(w, h);
  if (mdcj_jpeg_bound(w, h) > (1ll << 30))
    return fail(MDCJ_ERR_SIZE, "mdcj_create: %d x %d has %lld blocks; a frame's bit offsets are 32-bit (bound <= 2^30)", w, h, nblocks);
  if (nblocks * max_frames > 0x7fffffffll)
    return fail(MDCJ_ERR_SIZE, "mdcj_create: %lld blocks x %d frames per call is 2^31 or more", nblocks, max_frames);
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return fail(MDCJ_ERR_NO_DEVICE, "mdcj_create: no HIP device");
  if (device >= count) return fail(MDCJ_ERR_NO_DEVICE, "mdcj_create: device %d of %d", device, count);
  if (device < 0 && hipGetDevice(&device) != hipSuccess) return fail(MDCJ_ERR_HIP, "mdcj_create: hipGetDevice failed");
  DeviceGuard dg(device);
  mdcj_encoder* e = new (std::nothrow) mdcj_encoder;
  if (!e) return fail(MDCJ_ERR_NOMEM, "mdcj_create: out of host memory");
  e->device = device, e->w = w, e->h = h, e->quality = quality, e->max_frames = max_frames;
  e->nblocks = (int)nblocks;
  // ceil(1658 * nblocks / 32) words hold the longest stream; jenc_scan_kernel clears up to two more
  e->stream_words = ((long long)kBitsPerBlockMax * nblocks + 31) / 32 + 2;
  const size_t n = (size_t)nblocks * (size_t)max_frames;
  if (hipMalloc((void**)&e->d_tab, sizeof(DeviceTables)) != hipSuccess || hipMalloc((void**)&e->d_coef, n * 64 * sizeof(int16_t)) != hipSuccess ||
      hipMalloc((void**)&e->d_bits, n * sizeof(uint32_t)) != hipSuccess || hipMalloc((void**)&e->d_frame_bits, (size_t)max_frames * sizeof(uint32_t)) != hipSuccess ||
      hipMalloc((void**)&e->d_stream, (size_t)e->stream_words * (size_t)max_frames * sizeof(uint32_t)) != hipSuccess) {
    (void)hipGetLastError();
    mdcj_destroy(e);
    return fail(MDCJ_ERR_NOMEM, "mdcj_create: could not allocate the scratch arrays of %d frames of %d x %d", max_frames, w, h);
  }
  DeviceTables tab;
  fill_tables(&tab, w, h, quality);
  if (hipMemcpy(e->d_tab, &tab, sizeof tab, hipMemcpyHostToDevice) != hipSuccess) {
    mdcj_destroy(e);
    return fail(MDCJ_ERR_HIP, "mdcj_create: copying the tables failed");
  }
  *out = e;
  return MDCJ_OK;
}

}  // extern "C"

namespace {

template <typename T>
int encode(const char* who, mdcj_encoder* e, const T* d_frames, int64_t frame_stride, int nframes, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
           void* stream) {
  if (!e) return fail(MDCJ_ERR_ARG, "%s: encoder is null", who);
  if (nframes < 0 || nframes > e->max_frames) return fail(MDCJ_ERR_ARG, "%s: %d frames, the encoder was made for 0..%d", who, nframes, e->max_frames);
  if (nframes == 0) return MDCJ_OK;
  if (!d_frames || !d_out || !d_sizes) return fail(MDCJ_ERR_ARG, "%s: null device pointer", who);
  if (frame_stride < (int64_t)e->w * e->h) return fail(MDCJ_ERR_ARG, "%s: frame_stride %lld is below %d x %d", who, (long long)frame_stride, e->w, e->h);
  const int64_t bound = mdcj_jpeg_bound(e->w, e->h);
  if (slot_bytes < bound) return fail(MDCJ_ERR_SIZE, "%s: slot_bytes %lld is below mdcj_jpeg_bound(%d, %d) = %lld", who, (long long)slot_bytes, e->w, e->h, (long long)bound);
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

int mdcj_encode_f32_device(mdcj_encoder* enc, const float* d_frames, int64_t frame_stride, int nframes, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
                           void* stream) {
  return encode("mdcj_encode_f32_device", enc, d_frames, frame_stride, nframes, d_out, slot_bytes, d_sizes, stream);
}

int mdcj_output_device(mdcj_encoder* enc, uint8_t** d_out, int64_t* slot_bytes, int32_t** d_sizes) {
  if (!enc || !d_out || !slot_bytes || !d_sizes) return fail(MDCJ_ERR_ARG, "mdcj_output_device: null argument");
  const int64_t bound = mdcj_jpeg_bound(enc->w, enc->h);
  if (!enc->d_out) {
    DeviceGuard dg(enc->device);
    uint8_t* o = nullptr;
    int32_t* z = nullptr;
    if (hipMalloc((void**)&o, (size_t)bound * (size_t)enc->max_frames) != hipSuccess || hipMalloc((void**)&z, (size_t)enc->max_frames * sizeof(int32_t)) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(o);
      return fail(MDCJ_ERR_NOMEM, "mdcj_output_device: could not allocate %d slots of %lld bytes", enc->max_frames, (long long)bound);
    }
    enc->d_out = o, enc->d_sizes = z;
  }
  *d_out = enc->d_out, *slot_bytes = bound, *d_sizes = enc->d_sizes;
  return MDCJ_OK;
}

int64_t mdcj_fetch(mdcj_encoder* enc, const uint8_t* d_out, int64_t slot_bytes, const int32_t* d_sizes, int nframes, uint8_t* h_out, int64_t h_capacity,
                   int32_t* h_sizes, void* stream) {
  if (!enc || !d_out || !d_sizes || !h_sizes) return fail(MDCJ_ERR_ARG, "mdcj_fetch: null argument");
  if (nframes < 0 || nframes > enc->max_frames) return fail(MDCJ_ERR_ARG, "mdcj_fetch: %d frames, the encoder was made for 0..%d", nframes, enc->max_frames);
  if (nframes == 0) return 0;
  DeviceGuard dg(enc->device);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemcpyAsync(h_sizes, d_sizes, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return fail(MDCJ_ERR_HIP, "mdcj_fetch: copying the sizes failed: %s", hipGetErrorString(hipGetLastError()));
  int64_t total = 0;
  for (int f = 0; f < nframes; f++) {
    if (h_sizes[f] <= 0 || h_sizes[f] > slot_bytes) return fail(MDCJ_ERR_SIZE, "mdcj_fetch: frame %d has size %d, the slot %lld", f, h_sizes[f], (long long)slot_bytes);
    total += h_sizes[f];
  }
  if (!h_out) return total;
  if (total > h_capacity) return fail(MDCJ_ERR_SIZE, "mdcj_fetch: %lld bytes, room for %lld", (long long)total, (long long)h_capacity);
  // one copy per file costs more than the bytes (a thousand copies of 100 KB): gather on the device, copy once
  if (total > enc->packed_capacity || !enc->d_offsets) {
    (void)hipFree(enc->d_packed);
    enc->d_packed = nullptr, enc->packed_capacity = 0;
    const long long want = total + total / 4 + 4096;
    if (hipMalloc((void**)&enc->d_packed, (size_t)want) != hipSuccess ||
        (!enc->d_offsets && hipMalloc((void**)&enc->d_offsets, ((size_t)enc->max_frames + 1) * sizeof(long long)) != hipSuccess)) {
      (void)hipGetLastError();
      return fail(MDCJ_ERR_NOMEM, "mdcj_fetch: could not allocate %lld bytes for the gathered files", want);
    }
    enc->packed_capacity = want;
  }
  long long* offsets = new (std::nothrow) long long[(size_t)nframes + 1];
  if (!offsets) return fail(MDCJ_ERR_NOMEM, "mdcj_fetch: out of host memory");
  long long at = 0;
  int largest = 0;
  for (int f = 0; f < nframes; f++) {
    offsets[f] = at;
    at += h_sizes[f];
    if (h_sizes[f] > largest) largest = h_sizes[f];
  }
  offsets[nframes] = at;
  hipError_t err = hipMemcpy(enc->d_offsets, offsets, ((size_t)nframes + 1) * sizeof(long long), hipMemcpyHostToDevice);
  delete[] offsets;
  if (err != hipSuccess) return fail(MDCJ_ERR_HIP, "mdcj_fetch: copying the offsets failed: %s", hipGetErrorString(err));
  const unsigned parts = (unsigned)((largest + 16 * 256 - 1) / (16 * 256));  // 16 bytes per thread
  for (int f0 = 0; f0 < nframes; f0 += 65535) {
    const unsigned nf = (unsigned)(nframes - f0 < 65535 ? nframes - f0 : 65535);
    jenc_gather_kernel<<<dim3(parts, nf), 256, 0, s>>>(d_out + (int64_t)f0 * slot_bytes, (long long)slot_bytes, enc->d_offsets + f0, enc->d_packed);
  }
  if ((err = hipGetLastError()) != hipSuccess || (err = hipMemcpyAsync(h_out, enc->d_packed, (size_t)total, hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (err = hipStreamSynchronize(s)) != hipSuccess)
    return fail(MDCJ_ERR_HIP, "mdcj_fetch: gathering the files failed: %s", hipGetErrorString(err));
  return total;
}

int mdcj_encode_u8_device(mdcj_encoder* enc, const uint8_t* d_frames, int64_t frame_stride, int nframes, uint8_t* d_out, int64_t slot_bytes, int32_t* d_sizes,
                          void* stream) {
  return encode("mdcj_encode_u8_device", enc, d_frames, frame_stride, nframes, d_out, slot_bytes, d_sizes, stream);
}

}  // extern "C"
