// getImages / getImagesDevice: a range of frames through decode pool -> per-device lanes -> pipelined GPU calls.
// A call gets what it needs of its reader in a BatchEnv; it knows nothing else of it.
#pragma once
#include <mutex>
#include <string>
#include <vector>

#include "ExposureImage.h"
#include "decode_pool.h"
#include "device_lanes.h"

struct mdc_device_outputs;

namespace mdc_host {

// ring of getImages: chunks of 32 (64 in JPEG stage 2) page-locked frame buffers, 256 in all.  Chunk k is on the GPU while
// the pool decodes chunks k+1 .. (up to 192 frames in flight): a decode thread that is slow on one frame delays only the
// chunk that frame is in, not the pipeline (two half-rings of 64 stalled on every straggler: 2.5-2.9 k frames/s)
enum { kRingFrames = 256 };  // page-locked decode buffers of getImages (335 MB at 1280x1024, 670 MB in stage 1 and for calls of > 256 frames in stage 2; first getImages)

// The classes of PNG streams (Decode::want_png_stream's bits) that getImagesDevice hands to the device decoder by default: those that beat
// the host decoder on the same box in the same session (profiles/r06_pngd_rate.txt)
enum { kPngClassLiteral = 1, kPngClassStored = 2, kPngClassOther = 4, kPngDefaultClasses = kPngClassLiteral };

struct ErrorSink {  // lastError(): written by the caller's thread, and by the lanes of a batch call through note()
  std::string text;
  std::mutex mu;
  void note(const std::string& e) {
    std::lock_guard<std::mutex> lk(mu);
    text = e;
  }
};

struct BatchEnv {
  const FrameSource& src;
  DecodePool& pool;
  int W, H, w, h;      // frames as they are stored / rectified
  size_t frame_bytes;  // of a decoded frame
  const std::vector<double>& timestamps;
  const std::vector<float>& exposures;
  ErrorSink& err;
  bool quiet;  // the batch behind getImage's lookahead: a frame that fails is reported when the caller asks for it
  // GPU JPEG stage: JPEG frames travel as coefficient records (2 bytes per pixel + table), the inverse DCT runs on the device
  int gpu_jpeg;  // 0: JPEG decoded on the host; 1: host Huffman + device inverse DCT; 2: device Huffman + inverse DCT
  // device PNG decoder, getImagesDevice only: 0 PNG decoded on the host, 1 the stream classes of kPngDefaultClasses, 2 every eligible one,
  // 3 every eligible one by libmdc_pngdx.so (parallel inflate for streams with matches)
  int gpu_png;
};

// The (empty) result image of frame `id`
ExposureImage* new_image(const BatchEnv& env, int id, bool rectify);

// Frames first .. first+count-1 on the lanes `use` (all with a context): results into out[i], or (dev) left in the caller's device
// arrays with valid[i] = 1.  Returns the number of frames produced.
int run_batch(const BatchEnv& env, const std::vector<Lane*>& use, int first, int count, bool rectify, unsigned flags, ExposureImage** out,
              const mdc_device_outputs* dev, unsigned char* valid);

}  // namespace mdc_host
