#include "prefetch_cache.h"

#include <algorithm>

namespace mdc_host {

void PrefetchCache::release() {
  for (Slot& s : slots_) s.mem.release();
  slots_.clear();
  in_use_ = -1;
}

void PrefetchCache::ensure_slots(size_t frame_bytes) {
  const size_t want = (size_t)std::max(prefetch, 0) + 2;
  if (slots_.size() == want) return;
  drain();
  release();
  slots_.assign(want, Slot());
  for (Slot& s : slots_) {
    s.mem.alloc(frame_bytes);
    s.d.dst = s.mem.p;
    s.d.cap = frame_bytes;
  }
}

void PrefetchCache::drain() {
  DecodePool::Lock lk = pool_.lock();
  pool_.wait(lk, [&] {
    for (const Slot& s : slots_)
      if (pool_.busy(s.d)) return false;
    return true;
  });
}

// pool's lock held: a slot that is neither being decoded nor lent to the caller and holds nothing of value -- empty, or a
// frame the caller has already had (oldest first).  Frames decoded ahead and not yet asked for are never
// evicted for another prefetch (force: the caller itself needs a slot -- then the one farthest ahead goes).
int PrefetchCache::free_slot(bool force) {
  int best = -1;
  for (size_t i = 0; i < slots_.size(); i++) {
    const Slot& s = slots_[i];
    if (pool_.busy(s.d) || (int)i == in_use_) continue;
    if (s.d.id < 0) return (int)i;
    if (!s.consumed) continue;
    if (best < 0 || s.stamp < slots_[(size_t)best].stamp) best = (int)i;
  }
  if (best < 0 && force)
    for (size_t i = 0; i < slots_.size(); i++)
      if (!pool_.busy(slots_[i].d) && (int)i != in_use_ && (best < 0 || slots_[i].d.id > slots_[(size_t)best].d.id)) best = (int)i;
  return best;
}

const Decode* PrefetchCache::fetch(int id, size_t frame_bytes) {
  ensure_slots(frame_bytes);
  int k = -1;
  bool mine = false;  // not in the cache: decode in this thread
  {
    DecodePool::Lock lk = pool_.lock();
    for (size_t i = 0; i < slots_.size(); i++)
      if (slots_[i].d.id == id) k = (int)i;
    if (k >= 0) {
      hits++;
      pool_.wait(lk, [&] { return pool_.done(slots_[(size_t)k].d); });
    } else {
      misses++;
      in_use_ = -1;
      k = free_slot(true);
      if (k < 0) pool_.wait(lk, [&] { return (k = free_slot(true)) >= 0; });  // every other slot is being decoded into: wait for one
      slots_[(size_t)k].d.id = id;
      pool_.claim(slots_[(size_t)k].d);
      mine = true;
    }
    in_use_ = k;
    slots_[(size_t)k].consumed = true;
    slots_[(size_t)k].stamp = ++clock_;
  }
  Decode& d = slots_[(size_t)k].d;
  if (mine) pool_.decode_here(d);
  if (prefetch > 0 && src_.size() > 1) {
    pool_.start();
    DecodePool::Lock lk = pool_.lock();
    for (int a = 1; a <= prefetch && id + a < src_.size(); a++) {
      bool have = false;
      for (const Slot& s : slots_)
        if (s.d.id == id + a) have = true;
      if (have) continue;
      const int f = free_slot();
      if (f < 0) break;
      Slot& s = slots_[(size_t)f];
      s.d.id = id + a;
      s.consumed = false;
      s.stamp = ++clock_;
      pool_.queue(s.d);
    }
    pool_.notify();
  }
  return &d;
}

}  // namespace mdc_host
