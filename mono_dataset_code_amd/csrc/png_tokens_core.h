// The token path of libmdc_pngdx.so (include/mdc_pngdx.h states the rule) as code that both compilers take: hipcc for
// pngdx_tokens_kernel, g++ for tests/native/pngdx_core.cpp.  A team of kThreads threads inflates one ordinary DEFLATE stream: block
// by block, a Huffman block window by window, a window subsequence by subsequence.
//
// Every phase between two barriers is a function phase(t, S, ...) of the thread index and the shared arrays.  A phase writes only what
// no other thread reads in the same phase, with one exception that is stated where it is made (jump()).  decode_image() strings the
// phases together through a Team: team.each(f) runs f(t) for every thread and ends with a barrier, team.each_or(f) also gives the OR
// of what the threads returned.  On the device a Team is the workgroup; in the CPU program it is a loop over t, ascending or
// descending -- the result may not depend on which.  What decode_image() reads between two phases is the same in every thread: shared
// values that the phase after does not write.
//
// decode_image() gives up (false) on whatever is not a valid stream of exactly F bytes; it never reads outside the stream, never writes at
// or past out[F] or src[F].  The caller then runs the sequential decoder from the start, which names the reason.
#ifndef MDC_PNG_TOKENS_CORE_H
#define MDC_PNG_TOKENS_CORE_H
#include "png_inflate_core.h"

namespace pngx {

constexpr int kThreads = 1024;
constexpr int kSubBits = 64;  // a thread's subsequence; a token (length code 15 + 5, distance code 15 + 13) is at most 48 bits
constexpr uint32_t kWindowBits = (uint32_t)kThreads * kSubBits;
constexpr uint32_t kEnd = 0xffffffffu, kErr = 0xfffffffeu;  // exit states that are no bit position
constexpr int kMaxJumpRounds = 26;  // a window has at most kWindowBits / 2 matches: chains of at most 2^15 links halve in every round
constexpr int PATH_TOKENS = 4;      // = MDCX_PATH_TOKENS
enum { BLOCK_GIVE_UP = 0, BLOCK_STORED = 1, BLOCK_HUFFMAN = 2 };

struct Shared {
  pngd::Work w;
  uint32_t entry[kThreads];    // where the thread's first token starts
  uint32_t exit[2][kThreads];  // the state behind its last token, double-buffered over the relaxation rounds
  uint32_t bytes[kThreads];    // output bytes of its tokens | 1 << 31 if one of them is a match
  uint32_t opos[kThreads];     // the scan: where its first output byte goes
  uint32_t part[kThreads / 64];
  uint32_t kind, final, data_bit, st_at, st_len;  // the block header's result
  uint32_t total, end_pos;                         // a window's output bytes; the bit behind the end-of-block code
  uint32_t first;                                  // the first subsequence whose exit is kEnd or kErr (nsub: none)
};

struct Image {
  const uint8_t* p;  // the zlib stream
  uint32_t n, F;
  uint8_t* out;   // F filtered bytes
  uint32_t* src;  // F source indices
};

// src[] is read in jump() while other threads of the team replace entries by entries further down the same chain: relaxed atomics on
// the device (whole words, either value is right); plain accesses in the one-thread CPU program.
#if defined(__HIP_DEVICE_COMPILE__)
#define PNGX_LOAD(ptr) __hip_atomic_load((ptr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define PNGX_STORE(ptr, v) __hip_atomic_store((ptr), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define PNGX_MIN(ptr, v) ((void)__hip_atomic_fetch_min((ptr), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
#else
#define PNGX_LOAD(ptr) (*(ptr))
#define PNGX_STORE(ptr, v) (*(ptr) = (v))
#define PNGX_MIN(ptr, v) ((void)(*(ptr) = *(ptr) < (v) ? *(ptr) : (v)))
#endif

// ------------------------------------------------------------------------------------------------ the token span

struct Span {
  uint32_t exit, bytes, end_pos;
  bool match, bad_distance;
};

// Whole tokens from bit `entry` while a token starts before `end`: a literal, or length code + extra bits + distance code + extra bits.
// exit: the position of the first token at or behind `end`, kEnd behind the end-of-block code (end_pos = the bit behind it), kErr for
// bits that are no token or that the stream does not have.  WRITE: the first byte goes to `at`; a literal is stored and is its own
// source; byte i of a match at q with distance d has the source q - d + i % d, a byte from before the match (the sequential copy's
// value, also where d is below the length); a match with d > q writes nothing (bad_distance).  The caller has checked the room.
template <bool WRITE>
PNGD_HD Span span(const pngd::Work& w, const Image& im, uint32_t entry, uint32_t end, uint32_t at) {
  pngd::Bits b;
  b.seek(im.p, im.n, entry);
  Span r = {0, 0, 0, false, false};
  uint32_t ex = 0, v;
  bool open = true;
  while (open && b.bitpos() < end) {  // a round takes at least one bit
    const int s = pngd::decode(w.lit, b);
    if (s < 0 || s > 285) {
      ex = kErr, open = false;
    } else if (s < 256) {
      if (WRITE) im.out[at + r.bytes] = (uint8_t)s, PNGX_STORE(&im.src[at + r.bytes], at + r.bytes);
      r.bytes++;
    } else if (s == 256) {
      ex = kEnd, open = false;
      r.end_pos = b.bitpos();
    } else {
      const int i = s - 257;
      const int lx = i < 8 || i == 28 ? 0 : (i >> 2) - 1;
      uint32_t len = i < 8 ? (uint32_t)i + 3u : i == 28 ? 258u : ((4u + (uint32_t)(i & 3)) << lx) + 3u;
      bool ok = true;
      if (lx) ok = b.take(lx, v), len += ok ? v : 0u;
      const int d = ok ? pngd::decode(w.dist, b) : -1;
      if (d < 0 || d > 29) ok = false;
      const int dx = !ok || d < 4 ? 0 : (d >> 1) - 1;
      uint32_t dist = !ok ? 1u : d < 4 ? (uint32_t)d + 1u : ((2u + (uint32_t)(d & 1)) << dx) + 1u;
      if (dx) ok = b.take(dx, v), dist += ok ? v : 0u;
      if (!ok) {
        ex = kErr, open = false;
      } else {
        if (WRITE) {
          const uint32_t q = at + r.bytes;
          if (dist > q) {
            r.bad_distance = true;
          } else {
            uint32_t from = q - dist;
            for (uint32_t k = 0; k < len; k++) {  // len <= 258
              PNGX_STORE(&im.src[q + k], from);
              from = from + 1 == q ? q - dist : from + 1;
            }
          }
        }
        r.bytes += len;
        r.match = true;
      }
    }
  }
  r.exit = open ? b.bitpos() : ex;
  return r;
}

// ------------------------------------------------------------------------------------------------ blocks

// Thread 0: the header of the block at bit `pos`, `done` output bytes so far.  Stored: S.st_at, S.st_len (inside the stream and the
// room).  Huffman: the codes in S.w, S.data_bit = the first token.  Anything wrong: BLOCK_GIVE_UP.
PNGD_HD void block_header(Shared& S, const Image& im, uint32_t pos, uint32_t done) {
  pngd::Bits b;
  b.seek(im.p, im.n, pos);
  uint32_t hdr, v;
  S.kind = BLOCK_GIVE_UP;
  if (!b.take(3, hdr)) return;
  S.final = hdr & 1;
  const uint32_t type = hdr >> 1;
  if (type == 3) return;
  if (type == 0) {
    b.align();
    if (!b.take(32, v)) return;
    const uint32_t len = v & 0xffffu, at = b.bitpos() >> 3;
    if (len != ((~v >> 16) & 0xffffu) || len > im.n - at || len > im.F - done) return;
    S.st_at = at, S.st_len = len, S.kind = BLOCK_STORED;
    return;
  }
  int nd = 0;
  if (type == 1) pngd::fixed_codes(S.w);
  else if (pngd::dynamic_header(S.w, b, &nd) != pngd::ST_OK) return;
  S.data_bit = b.bitpos(), S.kind = BLOCK_HUFFMAN;
}

// ------------------------------------------------------------------------------------------------ a window: relaxation

// The window [ws, ws + nb) has nsub subsequences of kSubBits (the last one may be shorter); ws is a token boundary.
PNGD_HD uint32_t sub_end(uint32_t ws, uint32_t nb, int t) { return ws + (nb - (uint32_t)t * kSubBits < (uint32_t)kSubBits ? nb : ((uint32_t)t + 1) * kSubBits); }

PNGD_HD void decode_sub(Shared& S, const Image& im, uint32_t ws, uint32_t nb, int t, uint32_t entry, int buf) {
  const Span r = span<false>(S.w, im, entry, sub_end(ws, nb, t), 0);
  S.entry[t] = entry, S.exit[buf][t] = r.exit, S.bytes[t] = r.bytes | (r.match ? 1u << 31 : 0u);
}

// The guess: a token starts at the subsequence's first bit (true for subsequence 0).
PNGD_HD void first_guess(Shared& S, const Image& im, uint32_t ws, uint32_t nb, uint32_t nsub, int t) {
  if ((uint32_t)t < nsub) decode_sub(S, im, ws, nb, t, ws + (uint32_t)t * kSubBits, 0);
  else S.entry[t] = kErr, S.exit[0][t] = kErr, S.bytes[t] = 0;
  if (t == 0) S.first = nsub;
}

// One round: a subsequence whose left neighbour's exit is a position other than its entry starts again from there.  Reads exit[cur]
// of the neighbour, writes exit[cur ^ 1] of its own.  A neighbour's kEnd or kErr is NOT taken over: until the neighbour's entry is the
// sequential decoder's, its kErr is what a wrong guess decodes to (with distance codes that is common), and taking it over would
// throw away a subsequence that may already hold the right state.  After round k (the guess is round 0) subsequence k holds the
// sequential decoder's state unless a subsequence before it ended in kEnd or kErr; when a round changes nothing, every entry is its
// neighbour's exit from subsequence 0 up to the first kEnd or kErr, which therefore is the sequential decoder's (first_end()).
PNGD_HD bool relax(Shared& S, const Image& im, uint32_t ws, uint32_t nb, uint32_t nsub, int t, int cur) {
  if ((uint32_t)t >= nsub) return false;
  const uint32_t want = t == 0 ? ws : S.exit[cur][t - 1];
  if (want >= kErr || want == S.entry[t]) {
    S.exit[cur ^ 1][t] = S.exit[cur][t];
    return false;
  }
  decode_sub(S, im, ws, nb, t, want, cur ^ 1);
  return true;
}

// S.first = the first subsequence that ends in kEnd or kErr: the minimum over the threads, in any order
PNGD_HD void first_end(Shared& S, uint32_t nsub, int t, int cur) {
  if ((uint32_t)t < nsub && S.exit[cur][t] >= kErr) PNGX_MIN(&S.first, (uint32_t)t);
}

// The output bytes of subsequence k that count: none behind the first kEnd or kErr (decoded with the wrong codes)
PNGD_HD uint32_t live_bytes(const Shared& S, int k) { return (uint32_t)k <= S.first ? S.bytes[k] & 0x7fffffffu : 0u; }
PNGD_HD bool live_match(const Shared& S, int k) { return (uint32_t)k <= S.first && (S.bytes[k] >> 31) != 0; }

// ------------------------------------------------------------------------------------------------ a window: output positions

// The inclusive sum of live_bytes over the threads 64 * (t / 64) .. t
PNGD_HD uint32_t sum_in_group(const Shared& S, int t) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t inc = live_bytes(S, t);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t other = __shfl_up(inc, o, 64);
    if ((t & 63) >= o) inc += other;
  }
  return inc;
#else
  uint32_t inc = 0;
  for (int k = t & ~63; k <= t; k++) inc += live_bytes(S, k);
  return inc;
#endif
}

PNGD_HD void scan_groups(Shared& S, int t) {
  const uint32_t inc = sum_in_group(S, t);
  S.opos[t] = inc;
  if ((t & 63) == 63) S.part[t >> 6] = inc;
}

// A window's bytes are at most kWindowBits / 2 * 258 < 2^24: no sum wraps
PNGD_HD void scan_finish(Shared& S, uint32_t done, int t) {
  uint32_t before = 0, total = 0;
  for (int k = 0; k < kThreads / 64; k++) {
    before += k < (t >> 6) ? S.part[k] : 0;
    total += S.part[k];
  }
  S.opos[t] = done + before + S.opos[t] - live_bytes(S, t);
  if (t == 0) S.total = total;
}

// ------------------------------------------------------------------------------------------------ a window: writing

// The thread's tokens again, now with their positions.  true: a distance reaches before the first output byte.
PNGD_HD bool write_tokens(Shared& S, const Image& im, uint32_t ws, uint32_t nb, uint32_t nsub, int t) {
  if ((uint32_t)t >= nsub || (uint32_t)t > S.first) return false;
  const Span r = span<true>(S.w, im, S.entry[t], sub_end(ws, nb, t), S.opos[t]);
  if (r.exit == kEnd) S.end_pos = r.end_pos;  // one thread at most: S.first
  return r.bad_distance;
}

// Pointer doubling over the window's bytes [o0, o0 + total).  A byte is resolved when its source is itself (a literal) or lies before
// o0 (final: an earlier window, an earlier block).  Otherwise its source is a byte of this window, and it takes that byte's source
// unless that byte is a literal.  The one phase whose reads and writes overlap: src[s] may be replaced while it is read -- by an
// entry further down the same chain, with the same root, so the fixed point is the same in any order and no round resolves less than
// the plain double-buffered step would.
PNGD_HD bool jump(const Image& im, uint32_t o0, uint32_t total, int t) {
  bool changed = false;
  for (uint32_t i = (uint32_t)t; i < total; i += kThreads) {
    const uint32_t p = o0 + i, s = PNGX_LOAD(&im.src[p]);
    if (s == p || s < o0) continue;
    const uint32_t s2 = PNGX_LOAD(&im.src[s]);
    if (s2 == s) continue;
    PNGX_STORE(&im.src[p], s2);
    changed = true;
  }
  return changed;
}

// Every match byte from its resolved source: a literal of this window or a final byte before it, never a byte written here
PNGD_HD void gather(const Image& im, uint32_t o0, uint32_t total, int t) {
  for (uint32_t i = (uint32_t)t; i < total; i += kThreads) {
    const uint32_t p = o0 + i, s = PNGX_LOAD(&im.src[p]);
    if (s != p) im.out[p] = im.out[s];
  }
}

PNGD_HD void copy_stored(const Image& im, uint32_t at, uint32_t len, uint32_t done, int t) {
  for (uint32_t i = (uint32_t)t; i < len; i += kThreads) im.out[done + i] = im.p[at + i];  // len <= 65535
}

// ------------------------------------------------------------------------------------------------ the whole stream

// true: im.out holds the F bytes of the stream, *end_byte = where its trailer starts.  Every loop is bounded by the stream: a block
// takes at least its three header bits, a window at least one token, the relaxation at most nsub rounds, the doubling kMaxJumpRounds.
template <class Team>
PNGD_HD bool decode_image(Team& team, Shared& S, const Image& im, uint32_t* end_byte) {
  if (pngd::zlib_header(im.p, im.n) != pngd::ST_OK) return false;
  const uint32_t end_all = im.n * 8u;
  uint32_t pos = 16, done = 0;
  for (;;) {
    team.each([&](int t) {
      if (t == 0) block_header(S, im, pos, done);
    });
    const uint32_t kind = S.kind, final = S.final;
    if (kind == BLOCK_GIVE_UP) return false;
    if (kind == BLOCK_STORED) {
      const uint32_t at = S.st_at, len = S.st_len;
      team.each([&](int t) { copy_stored(im, at, len, done, t); });
      done += len, pos = (at + len) * 8u;
    } else {
      uint32_t ws = S.data_bit;
      for (;;) {
        if (ws >= end_all) return false;  // the input ends inside the block
        const uint32_t nb = end_all - ws < kWindowBits ? end_all - ws : kWindowBits, nsub = (nb + kSubBits - 1) / kSubBits;
        team.each([&](int t) { first_guess(S, im, ws, nb, nsub, t); });
        int cur = 0;
        for (uint32_t round = 0; round < nsub; round++) {
          const bool changed = team.each_or([&](int t) { return relax(S, im, ws, nb, nsub, t, cur); });
          cur ^= 1;
          if (!changed) break;
        }
        team.each([&](int t) { first_end(S, nsub, t, cur); });
        const uint32_t last = S.exit[cur][S.first < nsub ? S.first : nsub - 1];
        if (last == kErr) return false;
        team.each([&](int t) { scan_groups(S, t); });
        team.each([&](int t) { scan_finish(S, done, t); });
        const uint32_t total = S.total;
        if (total > im.F - done) return false;  // before anything of the window is written
        if (team.each_or([&](int t) { return write_tokens(S, im, ws, nb, nsub, t); })) return false;
        if (team.each_or([&](int t) { return live_match(S, t); })) {
          bool open = true;
          for (int r = 0; open && r < kMaxJumpRounds; r++) open = team.each_or([&](int t) { return jump(im, done, total, t); });
          if (open) return false;  // (cannot be)
          team.each([&](int t) { gather(im, done, total, t); });
        }
        done += total;
        if (last == kEnd) {
          pos = S.end_pos;
          break;
        }
        ws = last;  // a token boundary behind this window
      }
    }
    if (final) break;
  }
  *end_byte = (pos + 7u) >> 3;
  return done == im.F;
}

}  // namespace pngx
#endif  // MDC_PNG_TOKENS_CORE_H
