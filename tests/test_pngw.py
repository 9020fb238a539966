"""The device PNG encoder on the GPU (include/mdc_pngw.h, capi.PngEncoder): every file equals tests/pngw_restatement.py byte for
byte and PIL decodes it to the input; the code builder on directed histograms; both depths and all filter settings on the small
shapes; the stored path and its block limits; reuse, streams, alignments, the sentinel bytes behind every file, a batch past
65,536 images, the float conversion and the argument limits."""
import ctypes
import io
import zipfile

import numpy as np
import pytest

import pngw_restatement as P

pytestmark = pytest.mark.gpu
PATTERN = 0xA5
FILTERS = (0, 1, 2, 3, 4, P.ADAPTIVE)
DTYPES = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}


def torch_():
    import torch

    return torch


def decode(png):
    from PIL import Image

    return np.array(Image.open(io.BytesIO(png)))


def device_encode(images, depth, filt, kind=None, enc=None, stream=None, in_offset=0, out_offset=0, slot=None, stride=None, max_images=None):
    """images: equal-shaped arrays, one call.  Laid out `stride` elements apart from byte in_offset of a device array; the files go
    slot bytes apart from byte out_offset of a pattern-filled array.  -> the files; checks that only [f * slot, f * slot + size) of
    every slot was written, that the input was not, and that the sizes behind the batch are untouched."""
    from mono_dataset_code_amd import capi

    torch = torch_()
    kind = kind or ("u8" if depth == 8 else "u16")
    dt = DTYPES[kind]
    n, (h, w) = len(images), images[0].shape
    stride = stride or w * h
    own = enc is None
    if own:
        enc = capi.PngEncoder(w, h, depth=depth, filter=filt, max_images=max_images or n, device=0)
    slot = slot or enc.bound
    host_in = np.full(in_offset + n * stride * dt().itemsize + 64, PATTERN, np.uint8)
    for i, img in enumerate(images):
        at = in_offset + i * stride * dt().itemsize
        host_in[at:at + w * h * dt().itemsize] = np.ascontiguousarray(img, dt).reshape(-1).view(np.uint8)
    d_in = torch.from_numpy(host_in).to("cuda:0")
    d_out = torch.full((out_offset + n * slot + 64,), PATTERN, dtype=torch.uint8, device="cuda:0")
    d_sizes = torch.full((n + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    assert d_in.data_ptr() % 256 == 0 and d_out.data_ptr() % 256 == 0
    torch.cuda.synchronize()
    enc.encode(d_in.data_ptr() + in_offset, n, kind=kind, stride=stride, d_out=d_out.data_ptr() + out_offset, slot_bytes=slot, d_sizes=d_sizes.data_ptr(),
               stream=stream)
    torch.cuda.synchronize()
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
    return files


def check(files, images, depth, filt, stored=None):
    """every file == the restatement and decodes to its image; -> the restatement's stored flags"""
    flags = []
    for f, (got, img) in enumerate(zip(files, images)):
        want, was_stored = P.encode(img, depth, filt)
        assert len(got) == len(want) and got == want, (f, img.shape, depth, filt, len(got), len(want), [i for i in range(min(len(got), len(want))) if got[i] != want[i]][:8])
        assert ((got[43] >> 1) & 3) == (0 if was_stored else 2)  # BTYPE of the first block
        back = decode(got)
        assert back.shape == img.shape and np.array_equal(back.astype(np.uint16), img.astype(np.uint16)), (f, img.shape, depth, filt)
        flags.append(was_stored)
    if stored is not None:
        assert flags == stored, flags
    return flags


def contents(w, h, depth, seed):
    """noise, a smooth ramp (the dynamic path), one value everywhere (two symbols), zeros"""
    rng = np.random.default_rng(seed)
    top = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    yy, xx = np.mgrid[0:h, 0:w]
    return [rng.integers(0, top + 1, (h, w)).astype(dt), ((xx * 3 + yy * 5) * (top // 255) + (xx * yy) % 7).astype(dt), np.full((h, w), top // 3, dt),
            np.zeros((h, w), dt), (((xx + yy) // 3) * (top // 85) % (top + 1)).astype(dt)]


# ------------------------------------------------------------------------------------------------ the code builder


def test_huffman_lengths_device_equals_the_restatement():
    from mono_dataset_code_amd import capi

    torch = torch_()
    for name, hist, limit in P.directed_histograms():
        d_hist = torch.tensor(np.asarray(hist, np.uint32).view(np.int32), dtype=torch.int32, device="cuda:0")
        d_len = torch.full((len(hist) + 16,), PATTERN, dtype=torch.uint8, device="cuda:0")
        capi.huffman_lengths_device(d_hist.data_ptr(), len(hist), limit, d_len.data_ptr())
        torch.cuda.synchronize()
        got = d_len.cpu().numpy()
        assert (got[len(hist):] == PATTERN).all()
        assert got[:len(hist)].tolist() == P.huffman_lengths(hist, limit), name


# ------------------------------------------------------------------------------------------------ files


@pytest.mark.parametrize("depth", [8, 16])
@pytest.mark.parametrize("filt", FILTERS)
def test_small_shapes_equal_the_restatement(depth, filt):
    """no left neighbour (w = 1), no upper row (h = 1), bpp 2 with a one-pixel row, rows that end inside a 16-byte unit, and a
    64 x 48; five contents per call"""
    seen = set()
    for w, h in [(w, h) for w in (1, 2, 3, 17) for h in (1, 2, 5)] + [(64, 48)]:
        imgs = contents(w, h, depth, seed=w * 100 + h)
        seen.update(check(device_encode(imgs, depth, filt), imgs, depth, filt))
    assert seen == {False, True}  # both the dynamic and the stored form occurred


def test_every_value_equally_often_takes_the_stored_path():
    img = P.every_value_image()
    data = P.filtered(img, 8, 0).tobytes()
    assert np.bincount(np.frombuffer(data, np.uint8), minlength=256).tolist() == [8] * 256
    files = device_encode([img, np.zeros_like(img)], 8, 0)
    check(files, [img, np.zeros_like(img)], 8, 0, stored=[True, False])
    assert len(files[0]) == P.png_bound(255, 8, 8)


def test_fibonacci_histogram_image_is_length_limited_on_the_device():
    """One row of 10,943 pixels whose 17 values occur 2, 3, 5, ... 4181 times: with the one type byte and the one end-of-block the
    counts are the first 19 Fibonacci numbers, Huffman's tree is 18 deep, and the code is cut to 15"""
    counts = P.fibonacci(19)
    pixels = np.repeat(np.arange(10, 27, dtype=np.uint8), counts[2:])
    assert pixels.size == 10943
    img = np.random.default_rng(8).permutation(pixels).reshape(1, -1)
    data = P.filtered(img, 8, 0).tobytes()
    assert sorted(np.bincount(np.frombuffer(data, np.uint8)).tolist() + [1])[-19:] == counts
    _, lengths = P.dynamic_block(data)
    assert max(lengths) == 15 and len([l for l in lengths if l]) == 19
    check(device_encode([img], 8, 0), [img], 8, 0, stored=[False])


@pytest.mark.parametrize("w,h", [(254, 257), (255, 256), (509, 257), (131070, 1)], ids=["F65535", "F65536", "F131070", "F131071"])
def test_stored_block_limits(w, h):
    """F = 65535: one block; 65536: a second block of one byte; 131070: two full blocks; 131071: a third of one byte"""
    F = h * (1 + w)
    assert F == {(254, 257): 65535, (255, 256): 65536, (509, 257): 131070, (131070, 1): 131071}[(w, h)]
    values = np.resize(np.arange(256, dtype=np.uint8), w * h)  # every value equally often (within one)
    img = np.random.default_rng(F).permutation(values).reshape(h, w)
    files = device_encode([img], 8, 0)
    check(files, [img], 8, 0, stored=[True])
    assert len(files[0]) == P.png_bound(w, h, 8) == 63 + F + 5 * ((F + 65534) // 65535)


def test_encoder_reused_with_shrinking_batches():
    """stale scratch: histograms, Adler sums, tables and offsets of the larger batch before"""
    from mono_dataset_code_amd import capi

    enc = capi.PngEncoder(17, 5, depth=16, filter=P.ADAPTIVE, max_images=5, device=0)
    for n, seed in ((5, 1), (3, 2), (1, 3)):
        imgs = contents(17, 5, 16, seed)[:n]
        check(device_encode(imgs, 16, P.ADAPTIVE, enc=enc), imgs, 16, P.ADAPTIVE)
    enc.close()


def test_no_images_is_no_work():
    from mono_dataset_code_amd import capi

    torch = torch_()
    enc = capi.PngEncoder(4, 4, max_images=2, device=0)
    d_out = torch.full((2 * enc.bound,), PATTERN, dtype=torch.uint8, device="cuda:0")
    d_sizes = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    enc.encode(None, 0, d_out=d_out.data_ptr(), slot_bytes=enc.bound, d_sizes=d_sizes.data_ptr())
    enc.encode(d_out.data_ptr(), 0, kind="f32", d_out=d_out.data_ptr(), slot_bytes=0, d_sizes=d_sizes.data_ptr())  # before any other check
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == PATTERN).all() and (d_sizes.cpu().numpy() == 0x5A5A5A5A).all()
    enc.close()


def test_on_a_stream_of_the_callers():
    torch = torch_()
    stream = torch.cuda.Stream(device="cuda:0")
    imgs = contents(64, 48, 8, seed=5)
    check(device_encode(imgs, 8, P.ADAPTIVE, stream=stream.cuda_stream), imgs, 8, P.ADAPTIVE)


def test_every_base_alignment():
    """input and output start at byte k of their arrays, k = 0..15, with an odd slot size: the stream's first byte meets every
    position inside a 32-bit word, in every slot"""
    imgs = contents(17, 5, 8, seed=6)[:3]
    wants = [P.encode(img, 8, P.ADAPTIVE)[0] for img in imgs]
    bound = P.png_bound(17, 5, 8)
    for k in range(16):
        files = device_encode(imgs, 8, P.ADAPTIVE, in_offset=k, out_offset=k, slot=(bound | 1) + 2 * (k % 3), stride=17 * 5 + k)
        assert files == wants, k
    imgs16 = contents(3, 5, 16, seed=7)[:3]
    wants = [P.encode(img, 16, 4)[0] for img in imgs16]
    for k in range(0, 16, 2):  # 16-bit input is 2-byte aligned; the output is not
        assert device_encode(imgs16, 16, 4, in_offset=k, out_offset=k + 1, slot=P.png_bound(3, 5, 16) + k + 1) == wants, k


def test_batch_of_more_than_65536_images():
    """no kernel here keeps a 16-bit count of images (the grids are one-dimensional and strided): 65,537 images of 1 x 1"""
    n = 65537
    values = (np.arange(n) * 7919 % 256).astype(np.uint8)
    files = device_encode([v.reshape(1, 1) for v in values], 8, 0)
    want = {v: P.encode(np.array([[v]], np.uint8), 8, 0)[0] for v in range(256)}
    assert len(want[0]) == 70 == P.png_bound(1, 1, 8)
    bad = [f for f in range(n) if files[f] != want[int(values[f])]]
    assert not bad, bad[:10]
    assert decode(files[n - 1])[0, 0] == values[n - 1]


def test_f32_is_u8_of_the_converted_values():
    special = np.array([np.nan, np.inf, -np.inf, -0.4, 0.5, 1.5, 2.5, 254.5, 255.5, 1e10, -1e10, -0.0, 127.49, 127.5, 128.5, 3e9], np.float32)
    rng = np.random.default_rng(9)
    a = np.concatenate([special, rng.uniform(-20, 280, 16 * 5 - special.size).astype(np.float32)]).reshape(5, 16)
    b = (np.arange(80, dtype=np.float32) * 3.25 - 0.5).reshape(5, 16)  # many exact ties
    for filt in (0, P.ADAPTIVE):
        got = device_encode([a, b], 8, filt, kind="f32")
        as_u8 = [P.f32_to_u8(a), P.f32_to_u8(b)]
        assert got == device_encode(as_u8, 8, filt, kind="u8")
        check(got, as_u8, 8, filt)
    assert P.f32_to_u8(a).reshape(-1)[:12].tolist() == [0, 255, 0, 0, 0, 2, 2, 254, 255, 255, 0, 0]


def test_own_output_arrays_feed_the_zip_writer(tmp_path):
    """mdcp_output_device's slots and sizes are what mdcz_append_device takes"""
    from mono_dataset_code_amd import capi

    torch = torch_()
    imgs = contents(64, 48, 16, seed=10)
    enc = capi.PngEncoder(64, 48, depth=16, max_images=len(imgs), device=0)
    d_in = torch.from_numpy(np.stack(imgs).view(np.int16)).to("cuda:0")
    d_out, slot, d_sizes = enc.encode(d_in.data_ptr(), len(imgs), kind="u16")
    assert slot == enc.bound == P.png_bound(64, 48, 16)
    path = str(tmp_path / "images.zip")
    z = capi.ZipWriter(path, device=0)
    z.append(d_out, slot, d_sizes, len(imgs), first_index=3, suffix=".png")
    z.close()
    enc.close()
    with zipfile.ZipFile(path) as zf:
        assert zf.testzip() is None and zf.namelist() == ["%05d.png" % (3 + i) for i in range(len(imgs))]
        members = [zf.read(n) for n in zf.namelist()]
    check(members, imgs, 16, P.ADAPTIVE)


def test_every_argument_limit_is_a_status():
    from mono_dataset_code_amd import capi

    torch = torch_()
    L = capi.pngw_lib()
    err = lambda: L.mdcp_last_error().decode()  # noqa: E731
    h = ctypes.c_void_p()
    assert L.mdcp_create(99, 4, 4, 8, 0, 1, ctypes.byref(h)) == -5 and not h.value
    e8, e16 = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.mdcp_create(0, 4, 4, 8, 0, 2, ctypes.byref(e8)) == 0 and L.mdcp_create(-1, 4, 4, 16, P.ADAPTIVE, 2, ctypes.byref(e16)) == 0
    bound8, bound16 = L.mdcp_png_bound(4, 4, 8), L.mdcp_png_bound(4, 4, 16)
    d_in = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    d_out = torch.full((4 * bound16,), PATTERN, dtype=torch.uint8, device="cuda:0")
    d_sizes = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    i, o, z = d_in.data_ptr(), d_out.data_ptr(), d_sizes.data_ptr()
    u8, u16, f32 = L.mdcp_encode_u8_device, L.mdcp_encode_u16_device, L.mdcp_encode_f32_device
    assert u8(e8, i, 16, 3, o, bound8, z, None) == -1 and "0..2" in err()
    assert u8(e8, i, 16, -1, o, bound8, z, None) == -1
    assert u8(e8, None, 16, 1, o, bound8, z, None) == -1 and "null" in err()
    assert u8(e8, i, 16, 1, None, bound8, z, None) == -1 and u8(e8, i, 16, 1, o, bound8, None, None) == -1
    assert u8(e8, i, 15, 1, o, bound8, z, None) == -1 and "stride" in err()
    assert u8(e8, i, 16, 1, o, bound8 - 1, z, None) == -3 and "slot_bytes" in err()
    assert u16(e8, i, 16, 1, o, bound16, z, None) == -1 and "8-bit" in err()
    assert u8(e16, i, 16, 1, o, bound16, z, None) == -1 and f32(e16, i, 16, 1, o, bound16, z, None) == -1 and "16-bit" in err()
    assert u16(e16, i + 1, 16, 1, o, bound16, z, None) == -1 and "aligned" in err()
    assert f32(e8, i + 2, 16, 1, o, bound8, z, None) == -1 and "aligned" in err()
    assert u16(e16, i, 16, 1, o, bound16 - 1, z, None) == -3
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == PATTERN).all() and (d_sizes.cpu().numpy() == 0x5A5A5A5A).all()  # none of them did anything
    assert u16(e16, i, 16, 2, o, bound16, z, None) == 0  # and the encoders still work
    torch.cuda.synchronize()
    assert bytes(d_out.cpu().numpy()[:int(d_sizes.cpu().numpy()[0])]) == P.encode(np.zeros((4, 4), np.uint16), 16, P.ADAPTIVE)[0]
    L.mdcp_destroy(e8)
    L.mdcp_destroy(e16)
