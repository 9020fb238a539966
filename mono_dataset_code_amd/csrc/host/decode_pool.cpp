#include "decode_pool.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>

#include "image_codecs.h"
#include "image_codecs_internal.h"
#include "../png_inflate_core.h"
#include "mdc_hip.h"

namespace mdc_host {

void HostBuffer::alloc(size_t n) {
  p = static_cast<unsigned char*>(mdc_host_alloc(n));
  pinned = p != 0;
  if (!p) p = static_cast<unsigned char*>(std::malloc(n));
}
void HostBuffer::release() {
  if (!p) return;
  if (pinned) mdc_host_free(p);
  else std::free(p);
  p = 0;
}

// Never throws: it runs in the decode pool's threads, where an escaping exception (bad_alloc on a corrupt size field,
// ...) would terminate the process instead of reporting one bad frame.
void DecodePool::decode_now(Decode& d) const {
  try {
    decode_unguarded(d);
  } catch (const std::exception& e) {
    d.ok = false;
    d.err = std::string("decode failed: ") + e.what();
  } catch (...) {
    d.ok = false;
    d.err = "decode failed";
  }
}

void DecodePool::decode_unguarded(Decode& d) const {
  static thread_local std::vector<unsigned char> bytes;  // per-thread scratch, keeps its capacity between frames
  d.ok = false;
  d.w = d.h = 0;
  if (d.id < 0 || d.id >= src_.size()) {
    d.err = "frame index out of range";
    return;
  }
  if (!src_.read(d.id, bytes, &d.err)) return;
  d.is_record = d.is_stream = d.is_png_stream = false;
  if (d.want_png_stream && bytes.size() > 8 && bytes[0] == 0x89 && bytes[1] == 'P') {  // else, and for what is not eligible: pixels, below
    std::string why;
    size_t used = 0;
    if (png_stream(bytes.data(), bytes.size(), d.dst, d.cap, &used, &d.w, &d.h, &why) && used > 3) {
      // the class, by the device decoder's own rule (csrc/png_inflate_core.h: zlib header, first block header, its code lengths): a single
      // final dynamic block in which no distance symbol has a code; a first block that is stored; anything else
      static thread_local pngd::Work work;
      uint32_t data_bit = 0;
      const int path = pngd::classify(work, d.dst, (uint32_t)std::min<size_t>(used, pngd::kMaxStreamBytes), &data_bit);
      const unsigned cls = path == pngd::PATH_PARALLEL ? 1u : path == pngd::PATH_STORED ? 2u : 4u;
      if (d.want_png_stream & cls) {
        d.ok = d.is_png_stream = true;
        d.stream_bytes = used;
        return;
      }
    }
  }
  const bool is_jpeg = bytes.size() > 4 && bytes[0] == 0xff && bytes[1] == 0xd8;
  if (d.want_stream && is_jpeg) {  // what the device decoder takes (grayscale baseline, no restart markers); else the record path
    std::string why;
    size_t used = 0;
    if (jpeg_stream(bytes.data(), bytes.size(), d.dst, d.cap, &used, &d.w, &d.h, &why)) {
      d.ok = d.is_stream = true;
      d.stream_bytes = used;
      return;
    }
  }
  if (d.want_record_pitch > 0 && is_jpeg && d.cap > 256) {
    JpegCoefSink sink;
    sink.coef = reinterpret_cast<int16_t*>(d.dst + 128);
    sink.cap_blocks = (d.cap - 128) / 128;
    sink.pitch_blocks = d.want_record_pitch;
    d.ok = decode_jpeg_coefs(bytes.data(), bytes.size(), &sink, &d.err);
    if (d.ok) {
      std::memcpy(d.dst, sink.quant, 128);
      d.w = sink.w;
      d.h = sink.h;
      d.rec_rows = sink.blocks_rows;
      d.is_record = true;
    } else {
      // a file whose blocks do not fit the record geometry (or that the coefficient path refuses for any other reason)
      // still decodes to pixels on the host, so that stage 1 gives the same images and the same failures as stages 0 and 2
      std::string e2;
      d.ok = decode_gray8(bytes.data(), bytes.size(), d.dst, d.cap, &d.w, &d.h, &e2);
      if (!d.ok) d.err = e2;
    }
  } else {
    d.ok = decode_gray8(bytes.data(), bytes.size(), d.dst, d.cap, &d.w, &d.h, &d.err);
  }
  if (!d.ok) d.err = src_.name(d.id) + ": " + d.err;
}

void DecodePool::decode_here(Decode& d) {
  decode_now(d);
  std::lock_guard<std::mutex> lk(mu_);
  d.done_ = true;
}

void DecodePool::worker() {
  for (;;) {
    Decode* d = 0;
    {
      Lock lk(mu_);
      cv_job_.wait(lk, [&] { return stop_ || !jobs_.empty(); });
      if (stop_ && jobs_.empty()) return;
      d = jobs_.front();
      jobs_.pop_front();
    }
    decode_now(*d);
    {
      std::lock_guard<std::mutex> lk(mu_);
      d->busy_ = false;
      d->done_ = true;
    }
    cv_done_.notify_all();
  }
}

// (cgroup v2 cpu.max / v1 cpu.cfs_quota_us).  More decode threads than that only get throttled -- together with the
// HIP runtime's own threads (a box with 256 hardware threads and a 16-CPU quota decodes fastest with 16).
int DecodePool::usable_cpus() {
  unsigned hw = std::thread::hardware_concurrency();
  if (!hw) hw = 4;
  double quota = 0, period = 0;
  if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[64];
    if (std::fscanf(f, "%63s %lf", q, &period) == 2 && std::strcmp(q, "max") != 0) quota = std::atof(q);
    std::fclose(f);
  } else if (FILE* g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
    if (std::fscanf(g, "%lf", &quota) != 1) quota = 0;
    std::fclose(g);
    if (FILE* h = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
      if (std::fscanf(h, "%lf", &period) != 1) period = 0;
      std::fclose(h);
    }
  }
  if (quota > 0 && period > 0) hw = std::min<unsigned>(hw, std::max(1u, (unsigned)(quota / period + 0.5)));
  return (int)hw;
}

void DecodePool::start() {
  if (!workers_.empty()) return;
  const int n = want_threads_ > 0 ? want_threads_ : std::max(1, std::min(usable_cpus(), 64));
  for (int i = 0; i < n; i++) workers_.emplace_back(&DecodePool::worker, this);
}

void DecodePool::stop() {
  {
    std::lock_guard<std::mutex> lk(mu_);
    stop_ = true;
  }
  cv_job_.notify_all();
  for (auto& t : workers_) t.join();
  workers_.clear();
  stop_ = false;
}

void DecodePool::queue(Decode& d) {
  d.busy_ = true;
  d.done_ = false;
  jobs_.push_back(&d);
}

void DecodePool::submit(Decode* d, int n) {
  std::lock_guard<std::mutex> lk(mu_);
  for (int i = 0; i < n; i++) queue(d[i]);
  cv_job_.notify_all();
}

void DecodePool::wait_done(const Decode* d, int n) {
  Lock lk(mu_);
  cv_done_.wait(lk, [&] {
    for (int i = 0; i < n; i++)
      if (!d[i].done_) return false;
    return true;
  });
}

void DecodePool::wait_idle(const Decode* d, int n) {
  Lock lk(mu_);
  cv_done_.wait(lk, [&] {
    for (int i = 0; i < n; i++)
      if (d[i].busy_) return false;
    return true;
  });
}

}  // namespace mdc_host
