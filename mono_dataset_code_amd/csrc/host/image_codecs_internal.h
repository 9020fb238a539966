// What the decoders' translation units know of each other -- image_codecs.cpp (the dispatcher, PGM), image_codecs_png.cpp,
// image_codecs_jpeg.cpp, image_codecs_jpeg_stream.cpp -- and what gray_png.cpp (the vignette image), decode_pool.cpp and the C
// facade use of them.  Not installed.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace mdc_host {

inline bool fail(std::string* err, const char* msg) {
  if (err) *err = msg;
  return false;
}

struct PngAny {
  int w = 0, h = 0;
  int channels = 0;  // 1 gray, 2 gray + alpha, 3 RGB (also expanded palettes), 4 RGBA
  int bits = 0;      // 8 (1/2/4-bit gray already scaled to 8) or 16
  bool palette = false;
  std::vector<uint16_t> px;  // interleaved samples
};
bool png_decode_any(const unsigned char* data, size_t n, PngAny& im, std::string* err);
void png_any_to_gray8(const PngAny& im, unsigned char* out);  // w*h bytes, OpenCV's grayscale read of that PNG

// JPEG entropy decoding WITHOUT the inverse DCT: the quantised luma coefficients of a file, natural order, 64 int16 per
// 8x8 block, [blocks_rows][blocks_w][64] (the grid is padded to whole MCUs; the image covers the first ceil(h/8) rows and
// ceil(w/8) blocks of a row), + the luma quantisation table (natural order).  What the GPU stage of the reader takes
// (mdc_jpeg_idct_batch_device dequantises, inverts and crops on the device).  `coef` / `cap_blocks` are the caller's.
struct JpegCoefSink {
  int16_t* coef = nullptr;
  size_t cap_blocks = 0;
  int pitch_blocks = 0;  // in: row pitch in blocks the caller wants (0 = the file's own MCU-padded width)
  uint16_t quant[64];
  int w = 0, h = 0, blocks_w = 0, blocks_rows = 0;  // out: blocks_w = the row pitch used
};
bool decode_jpeg_coefs(const unsigned char* data, size_t n, JpegCoefSink* sink, std::string* err);

// GPU Huffman stage (include/mdc_hip.h: mdc_jpeg_stream_header): markers parsed, decode tables built, entropy-coded segment
// copied without its byte stuffing into `stream` (capacity cap) -- header, ecs bytes, 16 zero bytes; *used = bytes written.
// false (err says why) for what the device decoder does not take: more than one component, progressive / arithmetic /
// lossless files, restart intervals, 16-bit quantisation values above what a record holds, a stream that does not fit.
bool jpeg_stream(const unsigned char* data, size_t n, unsigned char* stream, size_t cap, size_t* used, int* w, int* h, std::string* err);

// The zlib stream of an 8-bit grayscale, non-interlaced PNG -- its IDAT bodies, concatenated -- copied to `stream`, for the device
// decoder (include/mdc_pngd.h).  false: any other flavour, no IHDR, a truncated chunk, or a stream that does not fit cap.
bool png_stream(const unsigned char* data, size_t n, unsigned char* stream, size_t cap, size_t* used, int* w, int* h, std::string* err);

// The format decoders behind decode_gray8 (image_codecs.h); a JPEG decoder with a sink delivers coefficients instead of samples.
bool png_gray8(const unsigned char* data, size_t n, unsigned char* out, size_t cap, int* w, int* h, std::string* err);
bool jpeg_gray8(const unsigned char* data, size_t n, unsigned char* out, size_t cap, int* w, int* h, std::string* err, JpegCoefSink* sink = nullptr);

}  // namespace mdc_host
