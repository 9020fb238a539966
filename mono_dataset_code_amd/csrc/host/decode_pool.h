// The reader's decode pool: worker threads that turn "frame id into this buffer" requests into pixels (or, for JPEG files and
// on request, into a coefficient record or an unstuffed stream for the device decoder).  One mutex guards the queue and
// publishes completions; no lock is held across a decode.
//
// Two ways in:
//   * ranges (getImages, getImagesRawDevice): submit(), wait_done(), wait_idle() -- requests of several threads share the queue;
//   * the lent lock (the prefetch cache): lock() hands out the pool's own mutex, so that the cache's slot bookkeeping is read and
//     written under the lock that publishes completions; queue() / notify() / wait() / busy() / done() work under it.
// Nobody outside touches the queue, the condition variables or a request's busy / done flags.
#pragma once
#include <condition_variable>
#include <cstddef>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "frame_source.h"

namespace mdc_host {

// One decode request: frame `id` into `dst`.  Filled in by whoever decodes it (a pool worker or the calling thread).
struct Decode {
  int id = -1;
  unsigned char* dst = 0;
  size_t cap = 0;
  int w = 0, h = 0;
  bool ok = false;
  // getImages with the GPU JPEG stage: a JPEG file is only Huffman-decoded, into a coefficient record at dst (pitch in blocks
  // as asked for); is_record tells what dst holds afterwards (other formats still decode to pixels)
  int want_record_pitch = 0;
  bool is_record = false;
  int rec_rows = 0;
  // ... or, with the Huffman decoding on the GPU as well, only unstuffed into a stream (mdc_jpeg_stream_header + bytes) at dst
  bool want_stream = false, is_stream = false;
  size_t stream_bytes = 0;
  // getImagesDevice with the device PNG decoder: an eligible PNG file (8-bit grayscale, non-interlaced, its first block of a class
  // in the mask: bit 0 a single final dynamic block in which no distance symbol has a code, bit 1 stored, bit 2 anything else) is only walked: its zlib
  // stream goes to dst (stream_bytes of it)
  unsigned want_png_stream = 0;
  bool is_png_stream = false;
  std::string err;

 private:
  friend class DecodePool;
  bool done_ = true, busy_ = false;  // busy: queued or being decoded; both published under the pool's mutex
};

struct HostBuffer {  // page-locked when a GPU is there, plain otherwise (decode works without a GPU)
  unsigned char* p = 0;
  bool pinned = false;
  void alloc(size_t n);
  void release();
};

class DecodePool {
 public:
  typedef std::unique_lock<std::mutex> Lock;

  explicit DecodePool(const FrameSource& src) : src_(src) {}
  ~DecodePool() { stop(); }

  // CPUs this process may actually use: the hardware threads, cut down to the container's CFS quota if there is one
  static int usable_cpus();
  int want_threads() const { return want_threads_; }  // 0: automatic (usable_cpus(), 64 at the most)
  void set_threads(int n) { want_threads_ = n; }      // takes effect at the next start(); stop() first
  int threads() const { return (int)workers_.size(); }
  void start();  // no-op while the workers run
  void stop();   // the workers finish what is queued, then end

  // Decodes in the calling thread.  Never throws: a failure is d.ok == false with d.err set.
  void decode_now(Decode& d) const;

  // ---- ranges ----
  void submit(Decode* d, int n);           // marks d[0..n) busy, queues them, wakes the workers
  void wait_done(const Decode* d, int n);  // until every one of d[0..n) is done
  void wait_idle(const Decode* d, int n);  // until none of d[0..n) is queued or being decoded (their storage may die then)

  // ---- the lent lock ----
  Lock lock() { return Lock(mu_); }
  bool busy(const Decode& d) const { return d.busy_; }
  bool done(const Decode& d) const { return d.done_; }
  void queue(Decode& d);                  // marks d busy and queues it; notify() once after the last one
  void notify() { cv_job_.notify_all(); }
  void claim(Decode& d) { d.done_ = false; }  // the caller decodes d itself: decode_here(d) after the lock is released
  template <class Pred>
  void wait(Lock& lk, Pred pred) { cv_done_.wait(lk, pred); }  // woken at every completion
  void decode_here(Decode& d);  // (lock NOT held) decode_now + publishing d as done

 private:
  void decode_unguarded(Decode& d) const;
  void worker();
  const FrameSource& src_;
  std::vector<std::thread> workers_;
  std::mutex mu_;
  std::condition_variable cv_job_, cv_done_;
  std::deque<Decode*> jobs_;
  bool stop_ = false;
  int want_threads_ = 0;
};

}  // namespace mdc_host
