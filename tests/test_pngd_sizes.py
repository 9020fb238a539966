"""The device PNG decoder (include/mdc_pngd.h, capi.PngDecoder) past its loops, tables and chain limits, on the inputs of
tests/pngd_problems.py: workgroups that decode a second and a third image of another kind, matches the whole wave copies at
distances and lengths around 64 and 258 and across blocks, codes of 15 bits in both alphabets, chains of 63, 64 and 65 stored
blocks, bytes after the trailer, a filter type in a late row, Adler sums of 2^20 large terms, 1024 single-bit mutations, streams
placed at odd addresses with sizes that lie, two calls queued back to back.  Every comparison is exact: pixels are PIL's, reason and
path the restatement's (tests/pngd_restatement.py), and no valid frame may come back with a reason.  tests/test_pngd_sizes_cpu.py
shows each input to be what it is taken for here, and runs every one of them through the kernels' core under the sanitizers first."""
import numpy as np
import pytest

import pngd_problems as Q
import pngd_restatement as R
from test_pngd import GAP, PATTERN, by_size, check_valid, device_decode, torch_

pytestmark = pytest.mark.gpu


def check_cases(cases):
    """cases of any sizes: the valid ones through check_valid, one call per size; the damaged ones through device_decode against the
    restatement -> {name: path}"""
    seen = {}
    valid = [(n, w, h, s) for n, w, h, s, reason, _ in cases if reason == R.OK]
    for (w, h), named in by_size(valid).items():
        for (name, _), path in zip(named, check_valid(w, h, named)):
            seen[name] = path
    damaged = [(n, w, h, (s, reason, path)) for n, w, h, s, reason, path in cases if reason != R.OK]
    for (w, h), named in by_size(damaged).items():
        frames, reasons, paths = device_decode(w, h, [s for _, (s, _, _) in named])
        for (name, (s, want, want_path)), frame, reason, path in zip(named, frames, reasons, paths):
            r_reason, r_path, _ = R.decode(s, w, h, pixels=False)
            assert reason == want == r_reason and frame is None, (name, R.REASONS[reason], R.REASONS[want])
            assert path == want_path == r_path, (name, path, want_path)
            seen[name] = path
    assert {name: path for name, _, _, _, _, path in cases} == seen
    return seen


# ------------------------------------------------------------------------------------------------ a workgroup's second and third image


def test_grid_stride_reuse_after_every_kind_of_image():
    """2 * 8192 + 64 frames in one call: the grid is capped at 8192, so workgroup b decodes the frames b, b + 8192 and (b < 64)
    b + 16384, and the workgroups 0 to 63 meet every ordered pair of the eight classes -- a stream of each path, valid and refused -- in
    LDS and registers another kind of image has left.  Then the same decoder again with the classes reversed: scratch and meta words a
    good frame has left are met by a refused one and the other way round."""
    from mono_dataset_code_amd import capi

    w, h, n = Q.CYCLE_W, Q.CYCLE_H, Q.CYCLE_FRAMES
    classes = Q.class_cycle()
    want = []
    for name, _, _, s, reason, path in classes:  # once per distinct stream
        r_reason, r_path, _ = R.decode(s, w, h, pixels=False)
        assert (r_reason, r_path) == (reason, path), name
        want.append((reason, path, R.pil_pixels(w, h, s) if reason == R.OK else None))
    dec = capi.PngDecoder(w, h, max_images=n, device=0)
    for reverse in (False, True):
        cls = [Q.cycle_class(f, reverse) for f in range(n)]
        assert set(cls) == set(range(8)) and {(cls[b], cls[b + 8192]) for b in range(64)} == {(a, b) for a in range(8) for b in range(8)}
        frames, reasons, paths = device_decode(w, h, [classes[c][3] for c in cls], dec=dec)  # refused frames keep their pattern bytes
        got = np.array([reasons, paths]).T
        assert np.array_equal(got, np.array([want[c][:2] for c in cls])), [(f, cls[f], got[f].tolist()) for f in range(n) if tuple(got[f]) != want[cls[f]][:2]][:10]
        wrong = [f for f in range(n) if want[cls[f]][2] is not None and not np.array_equal(frames[f], want[cls[f]][2])]
        assert wrong == [], (wrong[:10], [cls[f] for f in wrong[:10]])
    dec.close()


# ------------------------------------------------------------------------------------------------ the wave's copies, the slow decode


def test_match_grid_distances_and_lengths_around_64_and_258():
    """18 distances x 13 lengths, fixed codes, the general kernel: every match's source ends in a literal lane 0 has just stored, most
    overlap themselves (the copy takes the index modulo the distance), lengths of one, two, three, four and five rounds of 64 lanes"""
    seen = check_cases(Q.match_grid())
    assert len(seen) == 18 and set(seen.values()) == {R.GENERAL}


def test_matches_whose_source_another_block_wrote():
    seen = check_cases(Q.cross_block_matches())
    assert len(seen) == 3 and set(seen.values()) == {R.GENERAL}


def test_codes_of_15_bits_and_a_distance_code_of_one_bit():
    """both alphabets past the 9-bit table, in the general kernel, with length and distance symbols; a one-bit distance code and the bit
    that is no code of it; a literal-only header whose length symbol makes the parallel path give up"""
    ll, dl = Q.deep_code_lengths()
    assert max(ll) == 15 == max(dl)
    cases = Q.deep_codes()
    seen = check_cases(cases)
    assert [c[4] for c in cases] == [R.OK, R.OK, R.UNDEFINED_SYMBOL, R.UNDEFINED_SYMBOL] and set(seen.values()) == {R.GENERAL}
    assert R.first_path(cases[3][3], 1 + cases[3][1]) == R.PARALLEL


# ------------------------------------------------------------------------------------------------ chains, trailers, late rows, large sums


def test_stored_chains_at_the_block_limit():
    cases = Q.stored_chains()
    seen = check_cases(cases)
    assert [seen[c[0]] for c in cases] == [R.STORED, R.STORED, R.GENERAL, R.GENERAL, R.GENERAL]


def test_bytes_after_the_trailer_are_ignored_on_every_path():
    """... 8000 of them behind a literal-only stream: the parallel path's end state crosses some 950 subsequences, one a round when the
    bytes are zero (random ones hold end-of-block codes of their own)"""
    seen = check_cases(Q.trailing_bytes())
    assert sorted(seen.values()) == [R.PARALLEL] * 3 + [R.STORED] * 3 + [R.GENERAL] * 3


def test_filter_type_5_in_a_late_row():
    """rows 0, 255, 256 and 299 of 300: the check kernel's threads scan the rows 256 apart"""
    cases = Q.late_filter_types()
    assert [c[4] for c in cases] == [R.FILTER_TYPE] * 12
    seen = check_cases(cases)
    assert set(seen.values()) == {R.PARALLEL, R.STORED, R.GENERAL}


def test_adler_sums_of_a_megabyte_of_255():
    seen = check_cases(Q.heavy_adler())
    assert seen == {"heavy_stored": R.STORED, "heavy_literal": R.PARALLEL}


# ------------------------------------------------------------------------------------------------ single-bit damage


def test_mutation_sweep_equals_the_restatement():
    cases = Q.mutations()
    assert len(cases) == 1024
    frames, reasons, paths = device_decode(40, 12, [c[3] for c in cases])  # a frame with a reason keeps its pattern bytes
    wrong = [(c[0], R.REASONS[r], p, R.REASONS[c[4]], c[5]) for c, r, p in zip(cases, reasons, paths) if (r, p) != (c[4], c[5])]
    assert wrong == []
    refused = {(r, p) for r, p in zip(reasons, paths) if r}
    assert len({r for r, _ in refused}) >= 6 and {p for _, p in refused} == {R.PARALLEL, R.STORED, R.GENERAL}
    for c, frame in zip(cases, frames):
        if c[4] == R.OK:
            assert np.array_equal(frame, R.pil_pixels(40, 12, c[3])), c[0]


# ------------------------------------------------------------------------------------------------ where the streams and the frames lie


class Placed:
    """slot f holds files[f] cut to `slot` bytes, d_sizes is `sizes` as given, the frames start `frames_offset` bytes into a
    pattern-filled array.  launch() enqueues the call and does not wait; fetch() -> (frames or None, reasons, paths), every sentinel checked"""

    def __init__(self, dec, w, h, files, sizes, slot, frames_offset=GAP, stride=None, skip_head=0, skip_tail=0, slot_offset=0, stream=None):
        torch = torch_()
        self.dec, self.w, self.h, self.n, self.slot, self.slot_offset, self.frames_offset = dec, w, h, len(files), slot, slot_offset, frames_offset
        self.stride, self.kw = stride or w * h + GAP, dict(skip_head=skip_head, skip_tail=skip_tail, stream=stream)
        self.host = np.full(slot_offset + self.n * slot + 64, PATTERN, np.uint8)
        for f, data in enumerate(files):
            data = bytes(data)[:slot]
            self.host[slot_offset + f * slot:slot_offset + f * slot + len(data)] = np.frombuffer(data, np.uint8)
        self.d_slots = torch.from_numpy(self.host).to("cuda:0")
        self.d_sizes = torch.tensor(sizes, dtype=torch.int32, device="cuda:0")
        self.d_frames = torch.full((frames_offset + self.n * self.stride + GAP,), PATTERN, dtype=torch.uint8, device="cuda:0")
        self.d_status = torch.full((self.n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

    def launch(self):
        self.dec.decode_device(self.d_slots.data_ptr() + self.slot_offset, self.slot, self.d_sizes.data_ptr(), self.n, self.d_frames.data_ptr() + self.frames_offset,
                               self.d_status.data_ptr() + 16, frame_stride=self.stride, **self.kw)
        return self

    def fetch(self):
        from mono_dataset_code_amd import capi

        torch_().cuda.synchronize()
        n, w, h, stride, frames_offset = self.n, self.w, self.h, self.stride, self.frames_offset
        assert (self.d_slots.cpu().numpy() == self.host).all(), "the input was written to"
        status = self.d_status.cpu().numpy()
        assert (status[:4] == 0x5A5A5A5A).all() and (status[4 + n:] == 0x5A5A5A5A).all()
        reasons, paths = capi.PngDecoder.status_fields(status[4:4 + n])
        out = self.d_frames.cpu().numpy()
        assert (out[:frames_offset] == PATTERN).all() and (out[frames_offset + n * stride:] == PATTERN).all()
        frames = []
        for f in range(n):
            at = frames_offset + f * stride
            assert (out[at + w * h:at + stride] == PATTERN).all(), "frame %d: written behind its %d x %d bytes" % (f, w, h)
            frames.append(out[at:at + w * h].reshape(h, w).copy() if reasons[f] == 0 else None)
            assert reasons[f] == 0 or (out[at:at + w * h] == PATTERN).all(), "frame %d has a reason and pixels" % f
        return frames, reasons.tolist(), paths.tolist()


def raw_call(*a, **kw):
    return Placed(*a, **kw).launch().fetch()


def expect(streams, w, h):
    out = [R.decode(s, w, h) for s in streams]
    return [px for _, _, px in out], [r for r, _, _ in out], [p for _, p, _ in out]


def same(got, want):
    frames, reasons, paths = got
    assert (reasons, paths) == want[1:], [(f, a, b, c, d) for f, (a, b, c, d) in enumerate(zip(reasons, paths, want[1], want[2])) if (a, b) != (c, d)]
    for f, (a, b) in enumerate(zip(frames, want[0])):
        assert (a is None and b is None) or np.array_equal(a, b), f
    return True


def test_stream_placement_sizes_that_lie_and_frames_at_odd_addresses():
    from mono_dataset_code_amd import capi

    torch = torch_()
    w, h = 40, 12
    batch = Q.mixed_batch()
    streams = [s for _, s, _ in batch]
    n = len(streams)
    honest = expect(streams, w, h)
    assert honest[1] == [r for _, _, r in batch] and {R.PARALLEL, R.STORED, R.GENERAL} == {p for p, r in zip(honest[2], honest[1]) if r == 0}
    assert all(np.array_equal(px, R.pil_pixels(w, h, s)) for px, s in zip(honest[0], streams) if px is not None)
    dec = capi.PngDecoder(w, h, max_images=n, device=0)
    longest = max(len(s) for s in streams)
    # d_sizes above slot_bytes: the stream is the whole slot and no more (a slot_bytes that is no multiple of 4, slots from an odd address)
    whole = Q.clamped()
    assert Q.CLAMP_SLOT % 4 and Q.SLOT_FILL == PATTERN and [c[3] for c in whole] == [(s + bytes([PATTERN]) * 400)[:Q.CLAMP_SLOT] for s in streams]
    got = raw_call(dec, w, h, streams, [len(s) + 1000 * (1 + f % 3) for f, s in enumerate(streams)], Q.CLAMP_SLOT, slot_offset=1)
    assert same(got, expect([c[3] for c in whole], w, h)) and (got[1], got[2]) == ([c[4] for c in whole], [c[5] for c in whole])
    assert got[1].count(0) >= 6 and sum(r != r0 for r, r0 in zip(got[1], honest[1])) >= 6  # streams that still fit, and streams cut short
    # negative sizes: streams of no bytes
    sizes = [-1 if f % 3 == 0 else -2 ** 31 if f % 3 == 1 else len(s) for f, s in enumerate(streams)]
    got = raw_call(dec, w, h, streams, sizes, longest + 3)
    assert same(got, expect([s if f % 3 == 2 else b"" for f, s in enumerate(streams)], w, h))
    assert got[1][0] == got[1][1] == R.TRUNCATED and got[2][0] == got[2][1] == R.GENERAL
    # skip_head + skip_tail above the size: truncated, on the general path
    files = [b"\x01" * 41 + s + b"\x02" * 16 for s in streams]
    sizes = [len(f) if k % 2 else (0, 41, 56, 3)[k // 2 % 4] for k, f in enumerate(files)]
    got = raw_call(dec, w, h, files, sizes, longest + 57 + 2, skip_head=41, skip_tail=16)
    assert same(got, expect([s if k % 2 else b"" for k, s in enumerate(streams)], w, h))
    assert got[1][::2] == [R.TRUNCATED] * (n // 2) and got[2][::2] == [R.GENERAL] * (n // 2)
    # d_frames at odd addresses, one sentinel byte between two frames
    for offset in (1, 3):
        got = raw_call(dec, w, h, streams, [len(s) for s in streams], longest + 3, frames_offset=offset, stride=w * h + 1)
        assert same(got, honest), offset
    torch.cuda.synchronize()
    dec.close()


def test_two_calls_queued_on_one_stream_without_a_wait_between():
    """calls on one decoder are ordered by the caller; stream order is that order: the second call's kernels reuse the scratch only
    after the first call's unfilter has read it"""
    from mono_dataset_code_amd import capi

    torch = torch_()
    w, h = 40, 12
    streams = [s for _, s, _ in Q.mixed_batch()]
    first, second = streams, streams[::-1][3:]  # other streams in every slot, another count
    dec = capi.PngDecoder(w, h, max_images=len(first), device=0)
    side = torch.cuda.Stream()
    slot = max(len(s) for s in streams) + 3
    a = Placed(dec, w, h, first, [len(s) for s in first], slot, stream=side.cuda_stream)
    b = Placed(dec, w, h, second, [len(s) for s in second], slot, stream=side.cuda_stream)
    a.launch()  # everything is on the device and idle; from here to the second launch nothing waits
    b.launch()
    side.synchronize()
    assert same(a.fetch(), expect(first, w, h)) and same(b.fetch(), expect(second, w, h))
    dec.close()
