// class DatasetReader (include/mono_dataset_code/BenchmarkDatasetReader.h): the reference's sequence
// reader (src/BenchmarkDatasetReader.h:83-345) re-built around the fused GPU pass.
//
//   listing / log lines  : frame_source.cpp, as the reference (:86-125); folder or images.zip (zip_reader.cpp)
//   decode               : decode_pool.cpp -- own decoders (image_codecs.cpp) on a pool of worker threads, into page-locked buffers
//   getImageRaw          : prefetch_cache.cpp -- the frame asked for, and the pool decodes the ones after it
//   getImage             : one mdc_process_host call into a pooled page-locked ExposureImage; on a JPEG sequence read in
//                          order, results made ahead by getImages
//   getImages            : batch_run.cpp -- decode pool -> ring of page-locked chunks -> mdc_process_frames_host per chunk on
//                          every device's lane (device_lanes.cpp); the pool decodes the next chunks while chunk k is on the GPU
//
// This file: the constructor (times.txt (:282-324), calibration objects, frame size), the accessors and setters, and the public
// entry points on top of those units.
#include "BenchmarkDatasetReader.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "batch_run.h"
#include "device_lanes.h"
#include "host_device.h"
#include "mdc_hip.h"
#include "prefetch_cache.h"

using mdc_host::Decode;
using mdc_host::Lane;
using mdc_host::kRingFrames;

namespace {

unsigned flag_word(bool rectify, bool g, bool v, bool o) {
  return (rectify ? MDC_RECTIFY : 0u) | (g ? MDC_GAMMA : 0u) | (v ? MDC_VIGNETTE : 0u) | (o ? MDC_KILL_OVEREXPOSED : 0u);
}

}  // namespace

struct DatasetReader::State {
  std::string path;
  mdc_host::FrameSource src;
  mdc_host::DecodePool pool;
  mdc_host::PrefetchCache cache;
  mdc_host::DeviceLanes dev;
  std::vector<double> timestamps;
  std::vector<float> exposures;
  State() : pool(src), cache(pool, src) {}

  UndistorterFOV* fov = 0;
  PhotometricUndistorter* photo = 0;
  mdc_ctx* gpu = 0;  // lane 0's context
  int W = 0, H = 0, w = 0, h = 0;
  mdc_host::ErrorSink err;

  // frame size of a sweep folder without camera.txt (responseCalib needs only images + times.txt): the first decodable frame's
  int RW = 0, RH = 0;
  mdc_ctx* raw_gpu = 0;  // getImagesRawDevice's context when the reader has none of its own (no calibration to bind)
  size_t frame_bytes() const { return (size_t)frame_w() * frame_h(); }
  int frame_w() const { return W > 0 && H > 0 ? W : RW; }
  int frame_h() const { return W > 0 && H > 0 ? H : RH; }
  // GPU JPEG stage of getImages (batch_run.h).  Default on; MDC_GPU_JPEG=0 or setGpuJpeg(false) keeps the whole decode on the host.
  int gpu_jpeg = 2;
  // device PNG decoder of getImagesDevice (batch_run.h).  MDC_GPU_PNG=0 or setGpuPng(false) keeps PNG on the host.
  int gpu_png = 1;
  // getImage on a JPEG sequence read in order: after two consecutive ids the next `lookahead` frames go through the getImages
  // pipeline (Huffman decoding on the device) with the caller's switches, and the following calls hand those results out
  int lookahead = kRingFrames;  // the most; a run starts with 64 and doubles per batch (the longer the call, the less its fill and drain weigh)
  int ahead_batch = 64;
  std::vector<ExposureImage*> ahead;
  int ahead_first = -1;
  unsigned ahead_flags = 0;
  int seq_last = -2, seq_run = 0;
  bool quiet_batch = false;  // the batch behind getImage's lookahead: a frame that fails is reported when the caller asks for it
  void drop_ahead() {
    for (ExposureImage* e : ahead) delete e;
    ahead.clear();
    ahead_first = -1;
    ahead_batch = 64;
  }
  void note_id(int id) {  // how many ids in a row the caller has asked for
    seq_run = id == seq_last + 1 ? seq_run + 1 : 0;
    seq_last = id;
  }
  mdc_host::BatchEnv batch_env() {
    return mdc_host::BatchEnv{src, pool, W, H, w, h, frame_bytes(), timestamps, exposures, err, quiet_batch, gpu_jpeg, gpu_png};
  }
};

DatasetReader::DatasetReader(std::string folder) : s_(new State()) {
  if (const char* e = std::getenv("MDC_GPU_JPEG")) s_->gpu_jpeg = std::max(0, std::min(2, std::atoi(e)));
  if (const char* e = std::getenv("MDC_GPU_PNG")) s_->gpu_png = std::max(0, std::min(3, std::atoi(e)));
  if (const char* e = std::getenv("MDC_READER_LOOKAHEAD")) s_->lookahead = std::max(0, std::min((int)kRingFrames, std::atoi(e)));
  State& s = *s_;
  s.path = folder;
  s.src.open(s.path);

  // times.txt: "id stamp exposure" or "id stamp" per line (:282-324)
  {
    std::ifstream tr((s.path + "times.txt").c_str());
    std::string line;
    while (tr.good() && std::getline(tr, line)) {
      int id;
      double stamp;
      float exposure = 0;
      if (3 == std::sscanf(line.c_str(), "%d %lf %f", &id, &stamp, &exposure)) {
        s.timestamps.push_back(stamp);
        s.exposures.push_back(exposure);
      } else if (2 == std::sscanf(line.c_str(), "%d %lf", &id, &stamp)) {
        s.timestamps.push_back(stamp);
        s.exposures.push_back(0);
      }
    }
    if (s.exposures.size() != (size_t)s.src.size()) {
      std::printf("DatasetReader: Mismatch between number of images and number of timestamps / exposure times. Set all to zero.");
      s.timestamps.assign((size_t)s.src.size(), 0.0);
      s.exposures.assign((size_t)s.src.size(), 0.f);
    }
  }

  s.fov = new UndistorterFOV((s.path + "camera.txt").c_str());
  s.photo = new PhotometricUndistorter(s.path + "pcalib.txt", s.path + "vignette.png", s.fov->getInputDims()[0], s.fov->getInputDims()[1]);
  s.W = s.fov->getInputDims()[0];
  s.H = s.fov->getInputDims()[1];
  s.w = s.fov->getOutputDims()[0];
  s.h = s.fov->getOutputDims()[1];
  if (s.W <= 0 || s.H <= 0) {  // no (valid) camera.txt: the raw frames still have a size -- the first decodable frame's
    std::vector<unsigned char> buf;
    for (int id = 0; id < s.src.size() && !s.RW; id++) {
      Decode d;
      d.id = id;
      s.pool.decode_now(d);  // cap 0: fails, but a parsed header leaves the size behind
      if (d.w <= 0 || d.h <= 0) continue;
      buf.resize((size_t)d.w * d.h);
      d.dst = buf.data();
      d.cap = buf.size();
      s.pool.decode_now(d);
      if (d.ok) {
        s.RW = d.w;
        s.RH = d.h;
      }
    }
  }

  // one context holding BOTH objects' tables: the fused pass needs them together -- per device the reader may use
  // (MDC_DEVICES=all | 0,1,...; unset: the one device of $MDC_DEVICE / the calling thread, as before)
  s.gpu = s.dev.open(s.fov, s.photo);
  std::printf("Dataset %s: Got %d files!\n", s.path.c_str(), getNumImages());
}

DatasetReader::~DatasetReader() {
  State& s = *s_;
  s.pool.stop();
  s.cache.release();
  s.drop_ahead();
  s.dev.close();
  if (s.raw_gpu) mdc_destroy(s.raw_gpu);
  delete s.fov;
  delete s.photo;
  delete s_;
}

UndistorterFOV* DatasetReader::getUndistorter() { return s_->fov; }
PhotometricUndistorter* DatasetReader::getPhotoUndistorter() { return s_->photo; }
int DatasetReader::getNumImages() { return s_->src.size(); }
double DatasetReader::getTimestamp(int id) { return (id < 0 || id >= (int)s_->timestamps.size()) ? 0 : s_->timestamps[(size_t)id]; }
float DatasetReader::getExposure(int id) { return (id < 0 || id >= (int)s_->exposures.size()) ? 0 : s_->exposures[(size_t)id]; }
const char* DatasetReader::lastError() const { return s_->err.text.c_str(); }
void DatasetReader::getPrefetchStats(long* hits, long* misses) const {
  if (hits) *hits = s_->cache.hits;
  if (misses) *misses = s_->cache.misses;
}

// Devices in use = the lanes getImages deals its range to (one per entry of MDC_DEVICES).  The twin contexts that getImagesDevice adds on a
// device it already has a lane on are not devices of their own: their counters are folded into that lane's.
int DatasetReader::getDeviceCount() const { return s_->dev.device_count(); }
void DatasetReader::getDeviceStats(int lane, int* device, long* frames, double* decoder_wait_s, double* gpu_call_s) const {
  if (lane < 0 || lane >= getDeviceCount()) return;
  const std::vector<Lane>& lanes = s_->dev.lanes;
  const Lane& ln = lanes[(size_t)lane];
  long fr = ln.frames;
  double tw = ln.t_wait, tg = ln.t_gpu;
  bool first_of_device = true;
  for (int k = 0; k < lane; k++) first_of_device = first_of_device && lanes[(size_t)k].device != ln.device;
  if (first_of_device)  // (MDC_DEVICES=0,0: two host lanes on one device -- the twins go to the first of them)
    for (size_t k = (size_t)getDeviceCount(); k < lanes.size(); k++)
      if (lanes[k].twin && lanes[k].device == ln.device) {
        fr += lanes[k].frames;
        tw += lanes[k].t_wait;
        tg += lanes[k].t_gpu;
      }
  if (device) *device = ln.device;
  if (frames) *frames = fr;
  if (decoder_wait_s) *decoder_wait_s = tw;
  if (gpu_call_s) *gpu_call_s = tg;
}

void DatasetReader::setDecodeThreads(int n) {
  State& s = *s_;
  if (n < 0) n = 0;
  if (n == s.pool.want_threads()) return;
  s.cache.drain();
  s.pool.stop();
  s.pool.set_threads(n);
}

void DatasetReader::setResultLookahead(int frames) {
  s_->lookahead = std::max(0, std::min(frames, (int)kRingFrames));
  if (!s_->lookahead) s_->drop_ahead();
}
void DatasetReader::setGpuPng(bool on) { s_->gpu_png = on ? 1 : 0; }
void DatasetReader::setGpuPngMode(int mode) { s_->gpu_png = std::max(0, std::min(3, mode)); }
long DatasetReader::pngDeviceFrames() const {
  long n = 0;
  for (const mdc_host::Lane& ln : s_->dev.lanes) n += ln.png_frames;
  return n;
}
void DatasetReader::setGpuJpeg(bool on) { s_->gpu_jpeg = on ? 2 : 0; }
void DatasetReader::setGpuJpegStage(int stage) { s_->gpu_jpeg = std::max(0, std::min(2, stage)); }

void DatasetReader::setPrefetch(int frames) {
  s_->cache.prefetch = std::max(0, std::min(frames, 64));
}
const unsigned char* DatasetReader::getImageRaw(int id, int* width, int* height) {
  State& s = *s_;
  s.err.text.clear();
  if (id < 0 || id >= s.src.size()) {
    s.err.text = "frame index out of range";
    return 0;
  }
  const Decode* d = s.cache.fetch(id, s.frame_bytes());
  if (width) *width = d->w;
  if (height) *height = d->h;
  if (!d->ok) {
    s.err.text = d->err;
    return 0;
  }
  return d->dst;
}

ExposureImage* DatasetReader::getImage(int id, bool rectify, bool removeGamma, bool removeVignette, bool nanOverexposed) {
  State& s = *s_;
  if (id >= 0 && id < s.src.size() && s.gpu && s.lookahead > 0 && s.gpu_jpeg >= 2) {
    const unsigned flags = flag_word(rectify, removeGamma, removeVignette, nanOverexposed);
    if (!s.ahead.empty()) {  // results made ahead: hand this one out, or drop them when the caller went elsewhere
      const int k = id - s.ahead_first;
      if (flags == s.ahead_flags && k >= 0 && k < (int)s.ahead.size() && s.ahead[(size_t)k]) {
        ExposureImage* ret = s.ahead[(size_t)k];
        s.ahead[(size_t)k] = 0;
        if (k + 1 == (int)s.ahead.size()) {  // used up in order: the next batch is twice as long
          const int grown = std::min(2 * s.ahead_batch, (int)kRingFrames);
          s.drop_ahead();
          s.ahead_batch = grown;
        }
        s.note_id(id);
        return ret;
      }
      if (flags != s.ahead_flags || k < 0 || k >= (int)s.ahead.size()) s.drop_ahead();
    }
    s.note_id(id);
    if (s.ahead.empty() && s.seq_run >= 2 && s.src.is_jpeg_name(id)) {
      const int n = std::min(std::min(s.lookahead, s.ahead_batch), s.src.size() - id);
      s.ahead.assign((size_t)n, (ExposureImage*)0);
      s.quiet_batch = true;
      getImages(id, n, rectify, removeGamma, removeVignette, nanOverexposed, s.ahead.data());
      s.quiet_batch = false;
      s.ahead_first = id;
      s.ahead_flags = flags;
      if (s.ahead[0]) {
        ExposureImage* ret = s.ahead[0];
        s.ahead[0] = 0;
        if (n == 1) s.drop_ahead();
        return ret;
      }
      // (this frame failed in the batch: the single-frame path below says why, as the reference would)
    }
  }
  int fw = 0, fh = 0;
  const unsigned char* raw = getImageRaw(id, &fw, &fh);
  if (id < 0 || id >= s.src.size()) return 0;
  if (fh != s.H || fw != s.W) {  // also what an undecodable file leads to in the reference: an empty cv::Mat (:194-199)
    std::printf("ERROR: expected cv-mat to have dimensions %d x %d; found %d x %d (image %s)!\n", s.W, s.H, fw, fh,
                s.src.name(id).c_str());
    if (!raw && !s.err.text.empty()) std::fprintf(stderr, "DatasetReader: %s\n", s.err.text.c_str());
    return 0;
  }
  if (!raw) {
    std::fprintf(stderr, "DatasetReader: %s\n", s.err.text.c_str());
    return 0;
  }
  if (!s.gpu) {
    s.err.text = "no GPU context: the per-frame pass has no CPU fallback";
    std::fprintf(stderr, "DatasetReader::getImage: %s\n", s.err.text.c_str());
    return 0;
  }
  ExposureImage* ret = mdc_host::new_image(s.batch_env(), id, rectify);
  // the four switches are the library's flag word; every combination -- also "none" (plain cast, :234-240)
  // and "rectify only" (undistort<unsigned char>, :228-233) -- is one pass of the same kernel family
  if (mdc_process_host(s.gpu, raw, ret->image, flag_word(rectify, removeGamma, removeVignette, nanOverexposed)) != MDC_OK) {
    s.err.text = mdc_last_error(s.gpu);
    std::fprintf(stderr, "DatasetReader::getImage: %s\n", s.err.text.c_str());
    delete ret;
    return 0;
  }
  return ret;
}

int DatasetReader::getImages(int first, int count, bool rectify, bool removeGamma, bool removeVignette, bool nanOverexposed,
                             ExposureImage** out) {
  if (!out || count <= 0) return 0;
  return run_batch(first, count, rectify, removeGamma, removeVignette, nanOverexposed, out, 0, 0);
}

int DatasetReader::getImagesDevice(int first, int count, bool rectify, bool removeGamma, bool removeVignette, bool nanOverexposed,
                                   const mdc_device_outputs* out, unsigned char* valid) {
  if (!out || !out->base || count <= 0) {
    s_->err.text = "getImagesDevice: no device outputs";
    return 0;
  }
  return run_batch(first, count, rectify, removeGamma, removeVignette, nanOverexposed, 0, out, valid);
}

void DatasetReader::getRawSize(int* width, int* height) const {
  if (width) *width = s_->frame_w();
  if (height) *height = s_->frame_h();
}

// Raw frames for the responseCalib solver: the decode pool fills a page-locked block of up to 64 frames, which goes up frame by
// frame (contiguous runs of valid frames in one copy); the next block is decoded after the upload of the previous one.
int DatasetReader::getImagesRawDevice(int first, int count, int step, unsigned char* d_out, unsigned char* valid) {
  State& s = *s_;
  s.err.text.clear();
  if (count <= 0) return 0;
  if (valid) std::memset(valid, 0, (size_t)count);
  if (step < 1 || !d_out) {
    s.err.text = "getImagesRawDevice: bad argument";
    return 0;
  }
  const size_t fb = s.frame_bytes();
  if (!fb) {
    s.err.text = "getImagesRawDevice: no decodable frame, the frame size is unknown";
    return 0;
  }
  mdc_ctx* ctx = s.gpu;
  if (!ctx) {
    if (!s.raw_gpu) s.raw_gpu = mdc_host::open_device_context("DatasetReader");
    ctx = s.raw_gpu;
  }
  if (!ctx) {
    s.err.text = "getImagesRawDevice: no GPU";
    return 0;
  }
  const int kBatch = 64;
  const int per = std::min(kBatch, count);
  mdc_host::HostBuffer block;
  block.alloc((size_t)per * fb);
  std::vector<Decode> reqs((size_t)per);
  s.pool.start();
  int got = 0;
  for (int j0 = 0; j0 < count; j0 += per) {
    const int m = std::min(per, count - j0);
    for (int q = 0; q < m; q++) {
      Decode& d = reqs[(size_t)q];
      d = Decode();
      d.id = (int)std::min<long long>((long long)first + (long long)(j0 + q) * step, (long long)s.src.size());
      if (first < 0) d.id = -1;
      d.dst = block.p + (size_t)q * fb;
      d.cap = fb;
    }
    s.pool.submit(reqs.data(), m);
    s.pool.wait_done(reqs.data(), m);
    for (int q = 0; q < m;) {
      auto good = [&](int k) {
        const Decode& d = reqs[(size_t)k];
        return d.ok && d.w == s.frame_w() && d.h == s.frame_h();
      };
      if (!good(q)) {
        const Decode& d = reqs[(size_t)q];
        if (s.err.text.empty()) s.err.text = d.ok ? s.src.name(d.id) + ": wrong frame size" : d.err;
        q++;
        continue;
      }
      int r = q + 1;
      while (r < m && good(r)) r++;
      const int rc = mdc_copy_to_device(ctx, d_out + (size_t)(j0 + q) * fb, block.p + (size_t)q * fb, (size_t)(r - q) * fb);
      if (rc != MDC_OK) {
        s.err.text = std::string("getImagesRawDevice: ") + mdc_last_error(ctx);
        block.release();
        return got;
      }
      for (int k = q; k < r; k++)
        if (valid) valid[j0 + k] = 1;
      got += r - q;
      q = r;
    }
  }
  block.release();
  return got;
}

mdc_ctx* DatasetReader::getContext() { return s_->gpu; }
int DatasetReader::getDevice() const { return s_->gpu ? s_->dev.lanes[0].device : -1; }

// getImages (out) / getImagesDevice (dev, valid): the decode pool -> per-device lanes -> pipelined GPU calls (batch_run.cpp)
int DatasetReader::run_batch(int first, int count, bool rectify, bool removeGamma, bool removeVignette, bool nanOverexposed, ExposureImage** out,
                             const mdc_device_outputs* dev, unsigned char* valid) {
  State& s = *s_;
  s.err.text.clear();
  for (int i = 0; i < count && out; i++) out[i] = 0;
  for (int i = 0; i < count && valid; i++) valid[i] = 0;
  if (first < 0 || first + count > s.src.size()) {
    s.err.text = "frame range outside the sequence";
    return 0;
  }
  if (!s.gpu) {
    s.err.text = "no GPU context: the per-frame pass has no CPU fallback";
    std::fprintf(stderr, "DatasetReader::getImages: %s\n", s.err.text.c_str());
    return 0;
  }
  return mdc_host::run_batch(s.batch_env(), s.dev.for_batch(dev != 0), first, count, rectify, flag_word(rectify, removeGamma, removeVignette, nanOverexposed), out, dev, valid);
}
