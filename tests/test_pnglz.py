"""The device PNG encoder with LZ77 matches on the GPU (include/mdc_pnglz.h, capi.PngEncoder(compress="lz77")): every directed problem
of tests/pnglz_problems.py at chain 1, 4 and 64 equals tests/pnglz_restatement.py byte for byte, with its form and counts; a file
that does not take the match form is the Huffman-only encoder's file, made on the device in the same test, and none is larger than
that; sentinel bytes round every slot at every base alignment; a batch past 65,535 images; a 640 x 480 frame; two queued calls; the
float conversion; the project's own device decoder reads the match-form files; every error status."""
import ctypes
import io

import numpy as np
import pytest

import pnglz_problems as Q
import pnglz_restatement as Z
import pngw_restatement as P

pytestmark = pytest.mark.gpu
PATTERN = 0xA5
KINDS = {Z.GRAY8: ("u8", np.uint8, 1), Z.GRAY16: ("u16", np.uint16, 1), Z.RGB8: ("rgb8", np.uint8, 3)}


def torch_():
    import torch

    return torch


def decode(png):
    from PIL import Image

    return np.array(Image.open(io.BytesIO(png)))


def device_encode(images, kind, filt, chain=None, call="u8", enc=None, in_offset=0, out_offset=0, slot=None, stream=None, want_form=True):
    """images: equal-shaped arrays, one call; chain None: the Huffman-only encoder.  The files go `slot` bytes apart from byte
    out_offset of a pattern-filled array.  -> (the files, the form records or None); checks that only [f * slot, f * slot + size) of
    every slot was written and that the input was not."""
    from mono_dataset_code_amd import capi

    torch = torch_()
    name, dt, per = KINDS[kind]
    if call == "f32":
        name, dt = "f32", np.float32
    n, (h, w) = len(images), images[0].shape[:2]
    own = enc is None
    if own:
        enc = capi.PngEncoder(w, h, depth=16 if kind == Z.GRAY16 else 8, filter=filt, max_images=n, device=0, rgb=kind == Z.RGB8,
                              **({} if chain is None else {"compress": "lz77", "chain": chain}))
    slot = slot or enc.bound
    item = w * h * per * dt().itemsize
    host_in = np.full(in_offset + n * item + 64, PATTERN, np.uint8)
    for i, img in enumerate(images):
        host_in[in_offset + i * item:in_offset + (i + 1) * item] = np.ascontiguousarray(img, dt).reshape(-1).view(np.uint8)
    d_in = torch.from_numpy(host_in).to("cuda:0")
    d_out = torch.full((out_offset + n * slot + 64,), PATTERN, dtype=torch.uint8, device="cuda:0")
    d_sizes = torch.full((n + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    enc.encode(d_in.data_ptr() + in_offset, n, kind=name, d_out=d_out.data_ptr() + out_offset, slot_bytes=slot, d_sizes=d_sizes.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    forms = None
    if chain is not None and want_form:
        d_form = torch.full((n + 1, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        enc.form_device(d_form.data_ptr(), n, stream=stream)
        torch.cuda.synchronize()
        forms = d_form.cpu().numpy()
        assert (forms[n] == 0x5A5A5A5A).all()
        forms = forms[:n]
    if own:
        enc.close()
    sizes = d_sizes.cpu().numpy()
    out = d_out.cpu().numpy()
    assert (sizes[n:] == 0x5A5A5A5A).all()
    assert (d_in.cpu().numpy() == host_in).all(), "the input was written to"
    assert (out[:out_offset] == PATTERN).all()
    files = []
    for f in range(n):
        size = int(sizes[f])
        assert 0 < size <= enc.bound, (f, size)
        at = out_offset + f * slot
        end = out_offset + (f + 1) * slot if f + 1 < n else len(out)
        assert (out[at + size:end] == PATTERN).all(), "file %d: written behind its size" % f
        files.append(out[at:at + size].tobytes())
    return files, forms


def first_difference(a, b):
    return (len(a), len(b), [i for i in range(min(len(a), len(b))) if a[i] != b[i]][:8])


@pytest.mark.parametrize("chain", Q.CHAINS)
@pytest.mark.parametrize("name", [p[0] for p in Q.problems()])
def test_problem_equals_the_restatement(name, chain):
    _, img, kind, filt, _ = next(p for p in Q.problems() if p[0] == name)
    R = Q.restated(name)
    (got,), forms = device_encode([img], kind, filt, chain)
    want, info = R["file"][chain], R["info"][chain]
    assert got == want, (name, chain) + first_difference(got, want)
    assert tuple(int(v) for v in forms[0]) == info, (forms[0], info)
    (plain,), _ = device_encode([img], kind, filt, None)
    assert plain == R["huffman_only"]
    assert len(got) <= len(plain)
    if info[0] != Z.MATCHES:
        assert got == plain
    back = decode(got)
    assert back.shape == img.shape and np.array_equal(back.astype(np.uint16), img.astype(np.uint16))


def test_over_all_problems_no_file_is_larger_and_most_are_smaller():
    sizes = {}
    for name, img, kind, filt, _ in Q.problems():
        (got,), _ = device_encode([img], kind, filt, 4, want_form=False)
        (plain,), _ = device_encode([img], kind, filt, None)
        sizes[name] = (len(got), len(plain))
    assert all(a <= b for a, b in sizes.values()), sizes
    assert sum(a < b for a, b in sizes.values()) >= len(sizes) // 2, sizes


def test_sentinels_at_every_base_alignment_and_an_odd_slot():
    names = ("one_distance_symbol", "overlapping_source", "equal_lengths_nearest_wins")  # matches, matches, stored
    for name in names:
        _, img, kind, filt, _ = next(p for p in Q.problems() if p[0] == name)
        want = Q.restated(name)["file"][4]
        imgs = [img, img, img]
        for k in range(8):
            files, _ = device_encode(imgs, kind, filt, 4, in_offset=k, out_offset=k, slot=(P.png_bound(img.shape[1], img.shape[0], 8) | 1) + 2 * (k % 3))
            assert files == [want] * 3, (name, k)


def test_batch_of_70000_images():
    """past any 65,535 limit of a grid: 70,000 images of 5 x 3 cycling 16 contents"""
    rng = np.random.default_rng(11)
    contents = [np.full((3, 5), v, np.uint8) for v in range(4)] + [rng.integers(0, 4, (3, 5)).astype(np.uint8) for _ in range(8)] + \
               [rng.integers(0, 256, (3, 5)).astype(np.uint8) for _ in range(4)]
    want = [Z.encode(c, Z.GRAY8, P.ADAPTIVE, 4) for c in contents]
    assert {w[1][0] for w in want} == {Z.STORED, Z.HUFFMAN} and any(w[1][2] for w in want)  # so small, no match pays
    n = 70000
    files, forms = device_encode([contents[i % 16] for i in range(n)], Z.GRAY8, P.ADAPTIVE, 4)
    bad = [f for f in range(n) if files[f] != want[f % 16][0] or tuple(int(v) for v in forms[f]) != want[f % 16][1]]
    assert not bad, bad[:10]


_smooth = {}


def smooth(k):
    """(frame k of the rate tool's smooth workload, the restatement's file and record at chain 4), computed once"""
    from mono_dataset_code_amd import synth

    if k not in _smooth:
        img = synth.smooth_frame(640, 480, 0.3 * k, blobs=k % 2 == 0).reshape(480, 640)
        _smooth[k] = (img,) + Z.encode(img, Z.GRAY8, P.ADAPTIVE, 4)
    return _smooth[k]


def test_smooth_frame_640x480():
    img, want, info = smooth(0)
    (got,), forms = device_encode([img], Z.GRAY8, P.ADAPTIVE, 4)
    assert got == want, first_difference(got, want)
    assert tuple(int(v) for v in forms[0]) == info and info[0] == Z.MATCHES
    assert np.array_equal(decode(got), img)


def test_batch_of_640x480_frames():
    """16 frames in one call: the pack kernel then runs more workgroups than the device has compute units, several of an image side
    by side (a first version of it wrote wrong code bits into every image behind the fourth of such a batch)"""
    frames = [smooth(k % 2) for k in range(16)]
    files, forms = device_encode([f[0] for f in frames], Z.GRAY8, P.ADAPTIVE, 4)
    bad = [k for k in range(16) if files[k] != frames[k][1] or tuple(int(v) for v in forms[k]) != frames[k][2]]
    assert not bad, bad


def test_two_calls_queued_on_one_stream_without_a_wait():
    from mono_dataset_code_amd import capi

    torch = torch_()
    a = Q.bordered(Z.GRAY16, 40, 24, 1)
    b = np.zeros_like(a)
    enc = capi.PngEncoder(40, 24, depth=16, max_images=1, device=0, compress="lz77", chain=4)
    stream = torch.cuda.Stream(device="cuda:0")
    d_a, d_b = torch.from_numpy(a.view(np.int16)).to("cuda:0"), torch.from_numpy(b.view(np.int16)).to("cuda:0")
    outs = [torch.full((enc.bound,), PATTERN, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    sizes = [torch.zeros(1, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    for d, o, z in ((d_a, outs[0], sizes[0]), (d_b, outs[1], sizes[1])):
        enc.encode(d.data_ptr(), 1, kind="u16", d_out=o.data_ptr(), slot_bytes=enc.bound, d_sizes=z.data_ptr(), stream=stream.cuda_stream)
    torch.cuda.synchronize()
    for img, o, z in ((a, outs[0], sizes[0]), (b, outs[1], sizes[1])):
        assert o.cpu().numpy()[:int(z.cpu()[0])].tobytes() == Z.encode(img, Z.GRAY16, P.ADAPTIVE, 4)[0]
    enc.close()


def test_f32_is_u8_of_the_converted_values():
    special = np.array([np.nan, np.inf, -np.inf, -0.4, 0.5, 1.5, 2.5, 254.5, 255.5, 1e10, -1e10, -0.0, 127.49, 127.5, 128.5, 3e9], np.float32)
    a = np.concatenate([special, np.zeros(16 * 7, np.float32) + 300.0]).reshape(8, 16)
    as_u8 = P.f32_to_u8(a)
    (got,), forms = device_encode([a], Z.GRAY8, P.ADAPTIVE, 4, call="f32")
    (u8,), _ = device_encode([as_u8], Z.GRAY8, P.ADAPTIVE, 4)
    assert got == u8 == Z.encode(as_u8, Z.GRAY8, P.ADAPTIVE, 4)[0] and forms[0][0] == Z.MATCHES


def test_the_device_decoder_reads_the_match_form():
    from mono_dataset_code_amd import capi

    torch = torch_()
    imgs = [Q.bordered(Z.RGB8, 64, 48, s)[:, :, 0].copy() for s in (1, 2)] + [np.zeros((48, 64), np.uint8)]
    files, forms = device_encode(imgs, Z.GRAY8, P.ADAPTIVE, 4)
    assert (forms[:, 0] == Z.MATCHES).all()
    slot = max(len(f) for f in files) + 7
    host = np.zeros(len(files) * slot, np.uint8)
    for i, f in enumerate(files):
        host[i * slot:i * slot + len(f)] = np.frombuffer(f, np.uint8)
    d_slots = torch.from_numpy(host).to("cuda:0")
    d_sizes = torch.tensor([len(f) for f in files], dtype=torch.int32, device="cuda:0")
    d_frames = torch.full((len(files), 48, 64), PATTERN, dtype=torch.uint8, device="cuda:0")
    d_status = torch.full((len(files),), -1, dtype=torch.int32, device="cuda:0")
    dec = capi.PngDecoder(64, 48, max_images=len(files), device=0)
    # the zlib stream lies between byte 41 of the file and the 16 bytes of IDAT CRC and IEND
    dec.decode_device(d_slots.data_ptr(), slot, d_sizes.data_ptr(), len(files), d_frames.data_ptr(), d_status.data_ptr(), skip_head=41, skip_tail=16)
    torch.cuda.synchronize()
    reasons, _ = capi.PngDecoder.status_fields(d_status.cpu().numpy())
    assert (reasons == 0).all(), d_status.cpu().numpy()
    assert np.array_equal(d_frames.cpu().numpy(), np.stack(imgs))
    dec.close()


def test_every_argument_limit_is_a_status():
    from mono_dataset_code_amd import capi

    torch = torch_()
    L = capi.pnglz_lib()
    err = lambda: L.mdcl_last_error().decode()  # noqa: E731
    h = ctypes.c_void_p()
    assert L.mdcl_create(99, 4, 4, 0, 0, 4, 1, ctypes.byref(h)) == -5 and not h.value
    e8, e16, e24 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert L.mdcl_create(0, 4, 4, 0, 0, 4, 2, ctypes.byref(e8)) == 0 and L.mdcl_create(-1, 4, 4, 1, 5, 1, 2, ctypes.byref(e16)) == 0
    assert L.mdcl_create(0, 4, 4, 2, 5, 64, 2, ctypes.byref(e24)) == 0
    b8, b16, b24 = (L.mdcl_png_bound(4, 4, k) for k in (0, 1, 2))
    d_in = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    d_out = torch.full((4 * b24,), PATTERN, dtype=torch.uint8, device="cuda:0")
    d_sizes = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    i, o, z = d_in.data_ptr(), d_out.data_ptr(), d_sizes.data_ptr()
    u8, u16, f32, rgb = L.mdcl_encode_u8_device, L.mdcl_encode_u16_device, L.mdcl_encode_f32_device, L.mdcl_encode_rgb8_device
    assert u8(e8, i, 16, 3, o, b8, z, None) == -1 and "0..2" in err()
    assert u8(e8, i, 16, -1, o, b8, z, None) == -1
    assert u8(e8, None, 16, 1, o, b8, z, None) == -1 and "null" in err()
    assert u8(e8, i, 16, 1, None, b8, z, None) == -1 and u8(e8, i, 16, 1, o, b8, None, None) == -1
    assert u8(e8, i, 15, 1, o, b8, z, None) == -1 and "stride" in err()
    assert u8(e8, i, 16, 1, o, b8 - 1, z, None) == -3 and "slot_bytes" in err()
    assert u16(e8, i, 16, 1, o, b16, z, None) == -1 and "8-bit gray" in err()
    assert u8(e16, i, 16, 1, o, b16, z, None) == -1 and f32(e16, i, 16, 1, o, b16, z, None) == -1 and "16-bit gray" in err()
    assert rgb(e8, i, 48, 1, o, b24, z, None) == -1 and u8(e24, i, 16, 1, o, b24, z, None) == -1 and "RGB" in err()
    assert rgb(e24, i, 47, 1, o, b24, z, None) == -1 and "stride" in err() and rgb(e24, i, 48, 1, o, b24 - 1, z, None) == -3
    assert u16(e16, i + 1, 16, 1, o, b16, z, None) == -1 and "aligned" in err()
    assert f32(e8, i + 2, 16, 1, o, b8, z, None) == -1 and "aligned" in err()
    assert u16(e16, i, 16, 1, o, b16 - 1, z, None) == -3
    assert L.mdcl_kernel_ms(e8, (ctypes.c_float * 9)()) == -1 and "timed" in err()
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == PATTERN).all() and (d_sizes.cpu().numpy() == 0x5A5A5A5A).all()  # none of them did anything
    assert u8(e8, i, 16, 0, None, 0, None, None) == 0  # no images: no work, before any other check
    assert rgb(e24, i + 1, 48, 2, o, b24, z, None) == 0  # and the encoders still work, RGB input at any byte
    torch.cuda.synchronize()
    assert bytes(d_out.cpu().numpy()[:int(d_sizes.cpu().numpy()[0])]) == Z.encode(np.zeros((4, 4, 3), np.uint8), Z.RGB8, P.ADAPTIVE, 64)[0]
    for e in (e8, e16, e24):
        L.mdcl_destroy(e)
