"""The LZ77 PNG encoder on the GPU past every tile, chunk, chain and grid limit of its kernels: every input of tests/pnglz_limits.py
equals tests/pnglz_restatement.py byte for byte, with its form record, at the chains its property was asserted for by
tests/test_pnglz_sizes_cpu.py.  Single images: the sort tiles of pnglz_order_kernel, the rank blocks and the chain bound of
pnglz_match_kernel, every match length and every cap % 8 of common_prefix, the distance symbols 22..29, the scan's tiles, the filter
kernel past its 64-lane row loop.  Batches: 1024 and 1100 images of more than 16,384 bytes (the pack kernel with one workgroup per
1024 units), 524,291 small images (the parse kernel's grid-stride loop), the stored form past one 65,535-byte block, and an encoder
used again with other forms and fewer images."""
import numpy as np
import pytest

import pnglz_limits as M
import pnglz_restatement as Z
import pngw_restatement as P
from test_pnglz import PATTERN, decode, device_encode, first_difference, torch_

pytestmark = pytest.mark.gpu


def record(forms, f):
    return tuple(int(v) for v in forms[f])


@pytest.mark.parametrize("name", M.names())
def test_limit_equals_the_restatement(name):
    _, img, kind, filt, chains, _ = M.limit(name)
    R = M.restated(name)
    for chain in chains:
        (got,), forms = device_encode([img], kind, filt, chain)
        want = R["file"][chain]
        assert got == want, (name, chain) + first_difference(got, want)
        assert record(forms, 0) == R["info"][chain], (name, chain, forms[0], R["info"][chain])
    back = decode(got)
    assert back.shape == img.shape and np.array_equal(back.astype(np.uint16), img.astype(np.uint16))


def test_f32_past_the_row_loop_is_u8_of_the_converted_values():
    a = M.f32_image()
    as_u8 = P.f32_to_u8(a)
    (got,), forms = device_encode([a], Z.GRAY8, P.ADAPTIVE, 4, call="f32")
    (u8,), _ = device_encode([as_u8], Z.GRAY8, P.ADAPTIVE, 4)
    want, info = Z.encode(as_u8, Z.GRAY8, P.ADAPTIVE, 4)
    assert got == want, first_difference(got, want)
    assert u8 == want and record(forms, 0) == info and info[0] == Z.MATCHES


@pytest.mark.parametrize("n", M.PACK_CALLS)
def test_pack_kernel_with_one_workgroup_per_1024_units(n):
    """n >= 1024 images of 1032 units: two workgroups an image, every lane packs up to three units (the other tests have few images and
    many workgroups for each)"""
    frames = [M.pack_frame(k) for k in range(4)]
    files, forms = device_encode([frames[k % 4][0] for k in range(n)], Z.GRAY8, P.ADAPTIVE, 4)
    bad = [k for k in range(n) if files[k] != frames[k % 4][1] or record(forms, k) != frames[k % 4][2]]
    assert not bad, (len(bad), bad[:10], first_difference(files[bad[0]], frames[bad[0] % 4][1]))


def test_parse_kernel_past_its_grid():
    """8192 x 64 + 3 images of one chunk: the parse kernel's lanes take a second chunk.  Compared as arrays: every slot is its content's
    file and then the pattern."""
    from mono_dataset_code_amd import capi

    torch = torch_()
    contents = M.parse_contents()
    n, slot = M.PARSE_IMAGES, P.png_bound(5, 3, 8)
    which = np.arange(n) % 16
    want_slots = np.full((16, slot), PATTERN, np.uint8)
    for i, (_, png, _) in enumerate(contents):
        want_slots[i, :len(png)] = np.frombuffer(png, np.uint8)
    want_sizes = np.array([len(c[1]) for c in contents], np.int32)
    want_forms = np.array([c[2] for c in contents], np.int32)
    d_in = torch.from_numpy(np.stack([c[0].reshape(-1) for c in contents])[which].reshape(-1)).to("cuda:0")
    d_out = torch.full((n * slot + 64,), PATTERN, dtype=torch.uint8, device="cuda:0")
    d_sizes = torch.full((n + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    d_form = torch.full((n + 1, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    enc = capi.PngEncoder(5, 3, depth=8, filter=P.ADAPTIVE, max_images=n, device=0, compress="lz77", chain=4)
    assert enc.bound == slot
    enc.encode(d_in.data_ptr(), n, kind="u8", d_out=d_out.data_ptr(), slot_bytes=slot, d_sizes=d_sizes.data_ptr())
    enc.form_device(d_form.data_ptr(), n)
    torch.cuda.synchronize()
    enc.close()
    sizes, forms, out = d_sizes.cpu().numpy(), d_form.cpu().numpy(), d_out.cpu().numpy()
    assert (sizes[n:] == 0x5A5A5A5A).all() and (forms[n] == 0x5A5A5A5A).all() and (out[n * slot:] == PATTERN).all()
    bad = np.flatnonzero(sizes[:n] != want_sizes[which])
    assert bad.size == 0, (bad.size, bad[:10], sizes[bad[:10]])
    bad = np.flatnonzero((forms[:n] != want_forms[which]).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:10], forms[bad[:10]])
    out = out[:n * slot].reshape(n, slot)
    for i in range(16):  # 16 comparisons of 32,768 slots each
        rows = out[i::16]
        bad = np.flatnonzero((rows != want_slots[i]).any(axis=1))
        assert bad.size == 0, (i, bad.size, 16 * bad[:10] + i, first_difference(rows[bad[0]].tobytes(), want_slots[i].tobytes()))


@pytest.mark.parametrize("w,h", M.STORED_SHAPES)
def test_stored_form_past_one_block(w, h):
    """three images a call: the stored bytes of each are gathered by 16 or 32 workgroups; and the file is the Huffman-only encoder's"""
    images = M.stored_images(w, h)
    files, forms = device_encode([i[0] for i in images], Z.GRAY8, 0, 4)
    plain, _ = device_encode([i[0] for i in images], Z.GRAY8, 0, None)
    for k, (_, want, info) in enumerate(images):
        assert files[k] == want, (k,) + first_difference(files[k], want)
        assert record(forms, k) == info and info[0] == Z.STORED and plain[k] == want


def test_encoder_reused_with_other_forms_and_fewer_images():
    """stale scratch: the matches, offsets and table words of the call before; the scan skips stored images"""
    from mono_dataset_code_amd import capi

    enc = capi.PngEncoder(64, 48, depth=8, filter=P.ADAPTIVE, max_images=5, device=0, compress="lz77", chain=4)
    for c, call in enumerate(M.reuse_calls()):
        files, forms = device_encode([i[0] for i in call], Z.GRAY8, P.ADAPTIVE, 4, enc=enc)
        assert len(forms) == len(call)  # the records behind the call's images are not read
        for k, (_, want, info) in enumerate(call):
            assert files[k] == want, (c, k) + first_difference(files[k], want)
            assert record(forms, k) == info, (c, k, forms[k], info)
    enc.close()
