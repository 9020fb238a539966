// The prefetch cache of getImage / getImageRaw: a few frame-sized buffers; the frame asked for comes from one of them (decoded
// ahead by the pool, or decoded here), and the frames after it are queued.  The slots' bookkeeping (in_use, consumed, stamp)
// lives under the decode pool's own mutex, lent out by DecodePool::lock(): the one that publishes completions.
#pragma once
#include <vector>

#include "decode_pool.h"

namespace mdc_host {

class PrefetchCache {
 public:
  PrefetchCache(DecodePool& pool, const FrameSource& src) : pool_(pool), src_(src) {}
  ~PrefetchCache() { release(); }

  int prefetch = 16;         // frames decoded ahead after a fetch (0: none)
  long hits = 0, misses = 0;  // frames found decoded (or being decoded) ahead / decoded by the caller itself

  // The decoded frame `id` (from the cache, or decoded here), then the next frames are queued.  Valid until the next fetch.
  const Decode* fetch(int id, size_t frame_bytes);
  void drain();    // wait for every queued prefetch
  void release();  // the buffers go (the pool must be stopped or drained)

 private:
  struct Slot {
    Decode d;
    HostBuffer mem;
    bool consumed = true;  // already handed to the caller (or never filled)
    unsigned long stamp = 0;  // age
  };
  void ensure_slots(size_t frame_bytes);
  int free_slot(bool force = false);
  DecodePool& pool_;
  const FrameSource& src_;
  std::vector<Slot> slots_;
  int in_use_ = -1;  // slot whose buffer the caller holds (getImageRaw's promise)
  unsigned long clock_ = 0;
};

}  // namespace mdc_host
