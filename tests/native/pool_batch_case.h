// The reader's decode pool driven directly in the pattern of getImages (csrc/host/batch_run.cpp), without a GPU: shared by
// host_tsan.cpp and host_sanitize.cpp.  One owner holds the requests and their buffers; two lane threads deal the range's chunks
// between them, each submitting its own chunks two ahead and waiting on the sub-range of the chunk it consumes; on every other
// round lane 1 ends early and leaves requests queued, and the owner waits until none of the set is queued or busy before the
// storage dies (a late write of a worker into freed requests or buffers is what the sanitizers would report).
#pragma once
#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "decode_pool.h"
#include "frame_source.h"

// -> a checksum of what was decoded, or -1 if a frame that must decode did not (or `bad_frame` / an id past the end did)
static long pool_batch_case(const std::string& sequence_dir, int rounds, int bad_frame) {
  mdc_host::FrameSource src;
  src.open(sequence_dir);
  mdc_host::DecodePool pool(src);
  pool.set_threads(3);
  pool.start();
  const int n = src.size(), count = 4 * n + 3, C = 4, RG = 2, L = 2;  // 27 frames: 7 chunks, the last one short
  const size_t cap = 128 + 12 * 12 * 128;                             // a 48x32 frame, its stream or its coefficient record
  long sum = 0;
  bool wrong = false;
  for (int r = 0; r < rounds; r++) {
    std::vector<mdc_host::Decode> rec((size_t)count);
    std::vector<unsigned char> buffers((size_t)count * cap);
    const bool abandon = r % 2 == 1;
    auto lane = [&](int li, long* lane_sum, bool* lane_wrong) {
      const int nchunks = (count + C - 1) / C, mine = (nchunks - li + L - 1) / L;
      auto submit = [&](int j) {
        const int i0 = (li + j * L) * C, i1 = std::min(count, i0 + C);
        for (int i = i0; i < i1; i++) {
          mdc_host::Decode& d = rec[(size_t)i];
          d.id = i == count - 1 ? n : i % n;  // the last request is past the end of the sequence
          d.dst = &buffers[(size_t)i * cap];
          d.cap = cap;
          d.want_stream = r % 3 == 0;
          d.want_record_pitch = r % 3 == 1 ? 12 : 0;
        }
        pool.submit(&rec[(size_t)i0], i1 - i0);
      };
      for (int j = 0; j < std::min(mine, RG); j++) submit(j);
      if (abandon && li == 1) return;  // requests stay queued; rec and buffers are the owner's
      for (int j = 0; j < mine; j++) {
        const int i0 = (li + j * L) * C, i1 = std::min(count, i0 + C);
        pool.wait_done(&rec[(size_t)i0], i1 - i0);
        for (int i = i0; i < i1; i++) {
          const mdc_host::Decode& d = rec[(size_t)i];
          const bool must_fail = d.id >= n || d.id == bad_frame;
          if (d.ok == must_fail || (d.ok && (d.w != 48 || d.h != 32))) *lane_wrong = true;
          if (d.ok) *lane_sum += d.is_stream ? (long)d.stream_bytes : d.is_record ? d.rec_rows : d.dst[0] + d.dst[48 * 32 - 1];
        }
        if (j + RG < mine) submit(j + RG);
      }
    };
    long sums[2] = {0, 0};
    bool wrongs[2] = {false, false};
    std::thread helper(lane, 1, &sums[1], &wrongs[1]);
    lane(0, &sums[0], &wrongs[0]);
    helper.join();
    pool.wait_idle(rec.data(), count);
    sum += sums[0] + sums[1];
    wrong = wrong || wrongs[0] || wrongs[1];
  }
  return wrong ? -1 : sum;
}
