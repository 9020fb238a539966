#include "batch_run.h"

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <thread>

#include "mdc_hip.h"

namespace mdc_host {

ExposureImage* new_image(const BatchEnv& env, int id, bool rectify) {
  return new ExposureImage(rectify ? env.w : env.W, rectify ? env.h : env.H, env.timestamps[(size_t)id], env.exposures[(size_t)id], id);
}

namespace {

// The frames of a chunk that arrived in one form: their ring buffers, their result images' pixels (host results only) and their
// positions in the range (= in the caller's device arrays)
template <class Src>
struct FrameSet {
  std::vector<Src> src;
  std::vector<float*> dst;
  std::vector<int64_t> pos;
  void add(const unsigned char* buffer, ExposureImage* image, int i) {
    src.push_back(buffer);
    if (image) dst.push_back(image->image);
    pos.push_back(i);
  }
  void clear() {
    src.clear();
    dst.clear();
    pos.clear();
  }
  int64_t n() const { return (int64_t)src.size(); }
};
typedef FrameSet<const uint8_t*> PlainFrames;  // decoded pixels
typedef FrameSet<const void*> RecordFrames;    // JPEG coefficient records
struct StreamFrames : FrameSet<const void*> {  // JPEG streams (Huffman decoding on the device)
  std::vector<int64_t> bytes;
  std::vector<int> status;
  void clear() {
    FrameSet::clear();
    bytes.clear();
  }
};

struct PngFrames : FrameSet<const void*> {  // zlib streams of PNG files (inflate and unfilter on the device; getImagesDevice only)
  std::vector<long long> bytes;
  std::vector<int> status;
  void clear() {
    FrameSet::clear();
    bytes.clear();
  }
};

// What the lanes of one call share
struct Call {
  const BatchEnv& env;
  int first, count, C, RG, L;  // range; frames per chunk, chunks in a lane's ring, lanes
  bool rectify;
  unsigned flags;
  ExposureImage** out;
  const mdc_device_outputs* dev;  // getImagesDevice: results stay in the caller's device arrays (out == 0)
  unsigned char* valid;           // ... position i holds a result
  // coefficient records (include/mdc_hip.h): MCUs are 1..4 x 1..4 blocks, so a grid rounded up to multiples of 12 blocks
  // holds every sampling layout of a W x H file (the same rule as mdch_jpeg_record_bytes)
  int rec_pitch, rec_rows;
  size_t rec_bytes;
  std::vector<Decode> rec;
  std::mutex image_mu;
  const PngdApi* png;  // the device PNG decoder, where this call uses it
};

// One device of a sharded getImages call: chunks k = lane, lane + L, lane + 2L, ... of the range, each on the lane's own
// context, decode ring and GPU calls (reference src/BenchmarkDatasetReader.h:188-243: a frame depends on nothing but itself
// and the immutable tables, so the chunks of a range are independent).  The decode pool is shared; results land in the
// caller's order because every chunk writes its own slice of `out`.
struct LaneRun {
  Call& c;
  Lane& lane;
  int li;
  int produced = 0;
  int cur_i0 = 0, cur_i1 = 0;  // the chunk in flight: images allocated, pixels not (yet) written -- see drop_chunk_in_flight()
  double t_wait = 0, t_gpu = 0;
  LaneRun(Call& c_, Lane& lane_, int li_) : c(c_), lane(lane_), li(li_) {}

  static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  // the lane's j-th chunk is chunk li + j * L of the range; its buffers are ring position j % RG
  int chunk_begin(int j) const { return (li + j * c.L) * c.C; }
  int chunk_end(int j) const { return std::min(c.count, chunk_begin(j) + c.C); }
  void submit(int j) {
    const int i0 = chunk_begin(j), i1 = chunk_end(j);
    for (int i = i0; i < i1; i++) {
      Decode& d = c.rec[(size_t)i];
      d.id = c.first + i;
      d.dst = lane.ring_block.p + (size_t)((j % c.RG) * c.C + (i - i0)) * lane.ring_stride;
      d.cap = lane.ring_bytes;
      d.want_record_pitch = (c.env.gpu_jpeg && lane.ring_bytes >= c.rec_bytes) ? c.rec_pitch : 0;
      d.want_stream = c.env.gpu_jpeg >= 2;
      d.want_png_stream = !c.png ? 0u : c.env.gpu_png >= 2 ? (unsigned)(kPngClassLiteral | kPngClassStored | kPngClassOther) : (unsigned)kPngDefaultClasses;
    }
    c.env.pool.submit(&c.rec[(size_t)i0], i1 - i0);
  }
  // the frame of d is no result: says so as getImage would
  void bad_frame(const Decode& d) {
    if (!c.env.quiet)
      std::printf("ERROR: expected cv-mat to have dimensions %d x %d; found %d x %d (image %s)!\n", c.env.W, c.env.H, d.w, d.h, c.env.src.name(d.id).c_str());
    if (!d.ok) c.env.err.note(d.err);
    if (!d.ok) chunk_errors.push_back(std::make_pair(d.id - c.first, d.err));
  }
  // The chunk's failed frames (position, note).  A frame the device PNG decoder refuses fails after its neighbours have been looked at;
  // with such a frame in the chunk the note of the failure at the highest position is given once more at the chunk's end, so that
  // lastError() names the frame it names when the host decodes everything (one lane; several lanes note in the order they finish).
  std::vector<std::pair<int, std::string> > chunk_errors;
  bool late_failure = false;
  std::string png_error;  // the PNG decoder's own failure: the note of a chunk that fails for it
  bool fits(const Decode& d) const { return d.ok && d.w == c.env.W && d.h == c.env.H; }
  void give_back(int i) {  // position i holds no result (any more)
    if (c.out) {
      delete c.out[i];
      c.out[i] = 0;
    }
    if (c.valid) c.valid[i] = 0;
  }

  // The lane's PNG decoder, for n frames of the reader's size (0: none to be had -- the frames take the host decoder)
  void* png_decoder(int n) {
    if (lane.pngd && lane.pngd_from == c.png && lane.pngd_frames >= n) return lane.pngd;
    if (lane.pngd && lane.pngd_from) lane.pngd_from->destroy(lane.pngd);  // too small, or the other library's (the mode changed)
    lane.pngd = 0;
    const int want = std::max(n, c.C);
    if (c.png->create(lane.device, c.env.W, c.env.H, want, &lane.pngd) != 0) lane.pngd = 0;
    lane.pngd_from = lane.pngd ? c.png : 0;
    lane.pngd_frames = lane.pngd ? want : 0;
    return lane.pngd;
  }

  // PNG streams: inflated and unfiltered by libmdc_pngd.so into its own dense array, which the fused pass reads through the
  // device-pointer calls -- one per run of decoded frames at consecutive positions --, straight into the caller's arrays.  A stream
  // the device refuses (or all of them, without a decoder) goes to the host decoder, as a refused JPEG stream does.
  int run_png(PngFrames& png, int* refused) {
    const BatchEnv& env = c.env;
    const mdc_device_outputs* dev = c.dev;
    mdc_ctx* gpu = lane.gpu;
    const int n = (int)png.n();
    png.status.assign((size_t)n, -1);
    const unsigned char* d_frames = 0;
    void* dec = png_decoder(n);
    if (dec && c.png->decode_host(dec, png.src.data(), png.bytes.data(), n, png.status.data(), &d_frames) != 0) png.status.assign((size_t)n, -1);
    int grc = MDC_OK;
    if (dec && d_frames) {
      // The device-pointer calls enqueue on the stream they are given and do not wait.  This library has no HIP of its own to make or
      // wait for a stream, and mdc_synchronize covers only the context's internal streams: the fused pass therefore runs on the decoder's
      // stream (one per lane, so two lanes overlap) and mdci_synchronize waits for it; mdc_synchronize after it covers whatever the
      // context put on streams of its own.
      void* stream = c.png->stream(dec);
      const bool rect = (c.flags & MDC_RECTIFY) != 0, grads = dev->dI[0] != 0;
      const int w0 = rect ? env.w : env.W, h0 = rect ? env.h : env.H;
      const size_t n_in = (size_t)env.W * env.H, n_out = (size_t)w0 * h0;
      for (int q = 0; q < n && grc == MDC_OK;) {
        if ((png.status[(size_t)q] & 0xffff) != 0) {
          q++;
          continue;
        }
        const int64_t pos = png.pos[(size_t)q];
        int run = 1;
        while (q + run < n && (png.status[(size_t)(q + run)] & 0xffff) == 0 && png.pos[(size_t)(q + run)] == pos + run) run++;
        const uint8_t* src = d_frames + (size_t)q * n_in;
        float* base = dev->base + (size_t)pos * n_out;
        if (dev->levels == 1 && !grads) {
          grc = mdc_process_batch_device(gpu, src, base, run, c.flags, stream);
        } else {
          float *lv[3] = {0, 0, 0}, *gi[4] = {0, 0, 0, 0}, *ga[4] = {0, 0, 0, 0};
          for (int l = 0; l < dev->levels; l++) {
            const size_t npl = (size_t)(w0 >> l) * (size_t)(h0 >> l);
            if (l) lv[l - 1] = dev->level[l - 1] + (size_t)pos * npl;
            if (grads) gi[l] = dev->dI[l] + (size_t)pos * npl * 3, ga[l] = dev->abs_squared_grad[l] + (size_t)pos * npl;
          }
          grc = grads ? mdc_process_pyramid_gradients_batch_device(gpu, src, base, dev->levels, lv, gi, ga, run, c.flags, 0, stream)
                      : mdc_process_pyramid_batch_device(gpu, src, base, dev->levels, lv, run, c.flags, stream);
        }
        lane.png_frames += run;
        q += run;
      }
      if (c.png->synchronize(dec) != 0 && grc == MDC_OK) {
        png_error = std::string("getImagesDevice: PNG decoder: ") + c.png->last_error();
        return MDC_ERR_HIP;
      }
      if (grc == MDC_OK) grc = mdc_synchronize(gpu);
    }
    for (int q = 0; q < n && grc == MDC_OK; q++)
      if ((png.status[(size_t)q] & 0xffff) != 0) {  // the host decoder has the last word
        const int64_t pos = png.pos[(size_t)q];
        Decode one;
        one.id = c.first + (int)pos;
        one.dst = const_cast<unsigned char*>(static_cast<const unsigned char*>(png.src[(size_t)q]));  // the ring buffer of this frame
        one.cap = lane.ring_bytes;
        env.pool.decode_now(one);
        if (fits(one)) {
          const uint8_t* one_src = one.dst;
          grc = mdc_process_frames_host_to_device(gpu, &one_src, 1, c.flags, dev, &pos);
        } else {
          bad_frame(one);
          late_failure = true;
          give_back((int)pos);
          (*refused)++;
        }
      }
    return grc;
  }

  // run() threw (out of memory for an image or a list of pointers): the images it had made for the current chunk hold no
  // pixels yet and are not counted in `produced` -- a caller walking out[] for non-null entries must not meet them
  void drop_chunk_in_flight() {
    for (int i = cur_i0; i < cur_i1; i++) give_back(i);
    cur_i0 = cur_i1 = 0;
  }

  void run() {
    const BatchEnv& env = c.env;
    const mdc_device_outputs* dev = c.dev;
    const unsigned flags = c.flags;
    mdc_ctx* gpu = lane.gpu;
    const int nchunks = (c.count + c.C - 1) / c.C;
    const int mine = (nchunks - li + c.L - 1) / c.L;  // chunks of this lane
    for (int j = 0; j < std::min(mine, c.RG); j++) submit(j);
    PlainFrames plain;
    RecordFrames records;
    StreamFrames streams;
    PngFrames pngs;
    for (int j = 0; j < mine; j++) {
      const int i0 = chunk_begin(j), i1 = chunk_end(j);
      const double tw = now();
      env.pool.wait_done(&c.rec[(size_t)i0], i1 - i0);
      t_wait += now() - tw;
      cur_i0 = i0;
      cur_i1 = i1;
      plain.clear();
      records.clear();
      streams.clear();
      pngs.clear();
      chunk_errors.clear();
      late_failure = false;
      png_error.clear();
      {
        // a chunk's images are made in one go: the pool hands out consecutive blocks of a slab (lowest free address first),
        // and a chunk whose results lie back to back leaves the device with one copy -- another lane allocating in between
        // would interleave the two chunks' images
        std::lock_guard<std::mutex> alk(c.image_mu);
        for (int i = i0; i < i1; i++) {
          const Decode& d = c.rec[(size_t)i];
          if (!fits(d)) {
            bad_frame(d);
            continue;
          }
          if (c.out) c.out[i] = new_image(env, d.id, c.rectify);
          if (c.valid) c.valid[i] = 1;
          ExposureImage* image = c.out ? c.out[i] : 0;
          if (d.is_png_stream) {
            pngs.add(d.dst, image, i);
            pngs.bytes.push_back((long long)d.stream_bytes);
          } else if (d.is_stream) {
            streams.add(d.dst, image, i);
            streams.bytes.push_back((int64_t)d.stream_bytes);
          } else if (d.is_record) {
            if (d.rec_rows > c.rec_rows) {  // cannot happen while the decoder checks the sink's capacity: never hand a record on as pixels
              give_back(i);
              env.err.note(env.src.name(d.id) + ": coefficient record larger than the frame's geometry");
              continue;
            }
            records.add(d.dst, image, i);
          } else {
            plain.add(d.dst, image, i);
          }
        }
      }
      // chunk k on the GPU (uploads, kernels and downloads pipelined inside the call) while the pool decodes the next chunks
      const double tg = now();
      int refused = 0;  // streams neither the device nor the host decoder could read
      int grc = MDC_OK;
      if (plain.n())
        grc = dev ? mdc_process_frames_host_to_device(gpu, plain.src.data(), plain.n(), flags, dev, plain.pos.data())
                  : mdc_process_frames_host(gpu, plain.src.data(), plain.dst.data(), plain.n(), flags);
      if (grc == MDC_OK && records.n())  // records: Huffman-decoded on the host, inverse DCT on the device
        grc = dev ? mdc_process_jpeg_frames_host_to_device(gpu, records.src.data(), (int64_t)c.rec_bytes, c.rec_pitch, c.rec_rows, records.n(), flags, dev, records.pos.data())
                  : mdc_process_jpeg_frames_host(gpu, records.src.data(), (int64_t)c.rec_bytes, c.rec_pitch, c.rec_rows, records.dst.data(), records.n(), flags);
      if (grc == MDC_OK && streams.n()) {  // streams: Huffman decoding, inverse DCT and the fused pass on the device
        streams.status.assign((size_t)streams.n(), 0);
        grc = dev ? mdc_process_jpeg_streams_host_to_device(gpu, streams.src.data(), streams.bytes.data(), streams.n(), flags, dev, streams.pos.data(), streams.status.data())
                  : mdc_process_jpeg_streams_host(gpu, streams.src.data(), streams.bytes.data(), streams.dst.data(), streams.n(), flags, streams.status.data());
        for (size_t q = 0; q < streams.src.size() && grc == MDC_OK; q++)
          if (streams.status[q] != 0) {  // a stream the device could not decode (damaged file): the host decoder has the last word
            const int64_t pos = streams.pos[q];
            Decode one;
            one.id = c.first + (int)pos;
            one.dst = const_cast<unsigned char*>(static_cast<const unsigned char*>(streams.src[q]));  // the ring buffer of this frame
            one.cap = lane.ring_bytes;
            env.pool.decode_now(one);
            if (fits(one)) {
              const uint8_t* one_src = one.dst;
              grc = dev ? mdc_process_frames_host_to_device(gpu, &one_src, 1, flags, dev, &pos) : mdc_process_host(gpu, one.dst, c.out[pos]->image, flags);
            } else {
              bad_frame(one);
              give_back((int)pos);
              refused++;
            }
          }
      }
      if (grc == MDC_OK && pngs.n()) grc = run_png(pngs, &refused);
      t_gpu += now() - tg;
      if (late_failure && !chunk_errors.empty()) env.err.note(std::max_element(chunk_errors.begin(), chunk_errors.end())->second);
      if (grc != MDC_OK) {
        const std::string why = png_error.empty() ? std::string(mdc_last_error(gpu)) : png_error;
        env.err.note(why);
        std::fprintf(stderr, "DatasetReader::getImages: %s\n", why.c_str());
        for (int i = i0; i < i1; i++) give_back(i);
      } else {
        produced += (int)(plain.n() + records.n() + streams.n() + pngs.n()) - refused;
      }
      cur_i0 = cur_i1 = 0;  // the chunk is settled: its images are results (or gone)
      if (j + c.RG < mine) submit(j + c.RG);  // the buffers of the lane's chunk j are free again
    }
    lane.frames += produced;
    lane.t_wait += t_wait;
    lane.t_gpu += t_gpu;
  }
};

}  // namespace

int run_batch(const BatchEnv& env, const std::vector<Lane*>& use, int first, int count, bool rectify, unsigned flags, ExposureImage** out,
              const mdc_device_outputs* dev, unsigned char* valid) {
  // Frames per GPU call / calls in a lane's ring.  Stage 2 hands over up to a whole ring at a time -- its host work is ~0.1 ms
  // per frame and thread, and inside the GPU call a 64-frame chunk decodes while the one before it goes out: the longer the
  // call, the less its first decode and last output weigh (128 per call: 16.5 k frames/s, 256: 20+ k) -- and a lane with
  // more than one call gets a second ring's worth of buffers, so that the pool parses the next files while the GPU call of
  // the current ones runs (one ring: parse and GPU call take turns, 22 k frames/s).  With several devices (MDC_DEVICES) the
  // range is dealt to them in chunks of at least 64 frames, round-robin.
  const int L = (int)use.size();
  int C = env.gpu_jpeg >= 2 ? kRingFrames : 32;
  if (L > 1 && env.gpu_jpeg >= 2) C = std::min<int>(kRingFrames, std::max(64, ((count + L - 1) / L + 63) / 64 * 64));
  const int nchunks = (count + C - 1) / C;
  const int per_lane = (nchunks + L - 1) / L;
  const int slots = (env.gpu_jpeg >= 2 && per_lane > 1) ? 2 * C : (env.gpu_jpeg >= 2 ? C : kRingFrames), RG = slots / C;
  const int active = std::min(L, nchunks);
  const int rec_pitch = ((env.W + 7) / 8 + 11) / 12 * 12, rec_rows = ((env.H + 7) / 8 + 11) / 12 * 12;
  Call c = {env, first, count, C, RG, active, rectify, flags, out, dev, valid, rec_pitch, rec_rows, 128 + (size_t)rec_pitch * rec_rows * 128, {}, {}, (dev && env.gpu_png) ? pngd_api(env.gpu_png >= 3) : 0};
  // a ring buffer holds a decoded frame, or (stage 1) a coefficient record -- 2 bytes per pixel --, or (stage 2) a stream: the
  // compressed bytes + 5 KB; a file stage 2 does not take, or whose stream does not fit, is decoded to pixels on the host
  const size_t want_bytes = env.gpu_jpeg == 1 ? std::max(env.frame_bytes, c.rec_bytes) : env.frame_bytes;
  for (int l = 0; l < active; l++) {
    Lane& ln = *use[(size_t)l];
    if (!ln.ring_block.p || ln.ring_bytes < want_bytes || ln.ring_slots < slots) {
      ln.ring_block.release();
      ln.ring_stride = (want_bytes + 4095) & ~(size_t)4095;
      ln.ring_slots = slots;
      ln.ring_block.alloc(ln.ring_stride * (size_t)ln.ring_slots);
      ln.ring_bytes = want_bytes;
    }
  }
  env.pool.start();
  c.rec.resize((size_t)count);
  const bool trace = std::getenv("MDC_READER_TRACE") != 0;  // where a getImages call spends its time (stderr)
  std::vector<LaneRun> runs;
  runs.reserve((size_t)active);
  for (int l = 0; l < active; l++) runs.push_back(LaneRun(c, *use[(size_t)l], l));
  // every lane runs to its end whatever happens in another one (an exception -- out of memory for a list of pointers -- ends
  // that lane's chunks with an error, not the process: a std::thread must not be left joinable, a lane's images must not leak)
  auto run_lane = [&runs, &env](int l, bool helper_thread) {
    try {
      // only a helper thread of this call is pinned near its GPU: the caller's own thread -- lane 0, and any lane that runs here because no
      // thread could be made -- keeps the affinity the application gave it
      if (helper_thread) pin_thread_near_device(runs[(size_t)l].lane.gpu);
      runs[(size_t)l].run();
    } catch (const std::exception& e) {
      runs[(size_t)l].drop_chunk_in_flight();
      env.err.note(std::string("getImages: lane failed: ") + e.what());
    } catch (...) {
      runs[(size_t)l].drop_chunk_in_flight();
      env.err.note("getImages: lane failed");
    }
  };
  std::vector<std::thread> helpers;
  for (int l = 1; l < active; l++) {
    try {
      helpers.emplace_back(run_lane, l, true);
    } catch (...) {  // no thread to be had: the lane's chunks run here, after lane 0's
      helpers.emplace_back();
    }
  }
  run_lane(0, false);
  for (int l = 1; l < active; l++) {
    if (helpers[(size_t)(l - 1)].joinable()) helpers[(size_t)(l - 1)].join();
    else run_lane(l, false);
  }
  // `rec` dies with this call: no decode job may still point into it (a lane that ended early leaves some queued)
  env.pool.wait_idle(c.rec.data(), count);
  int produced = 0;
  for (const LaneRun& r : runs) produced += r.produced;
  if (trace)
    for (const LaneRun& r : runs)
      std::fprintf(stderr, "DatasetReader::getImages: device %d (lane %d of %d): %d of %d frames, %d decode threads: waited %.1f ms for the decoders, %.1f ms in the GPU calls\n",
                   r.lane.device, r.li, active, r.produced, count, env.pool.threads(), r.t_wait * 1e3, r.t_gpu * 1e3);
  if (trace && c.png) {
    long png_frames = 0;
    for (const LaneRun& r : runs) png_frames += r.lane.png_frames;
    std::fprintf(stderr, "DatasetReader::getImages: %ld PNG frames decoded on the device so far\n", png_frames);
  }
  return produced;
}

}  // namespace mdc_host
