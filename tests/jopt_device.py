"""What tests/test_jopt.py and tests/test_jopt_sizes.py share: one encode call of libmdc_jopt.so (include/mdc_jopt.h) through the raw
functions into pattern-filled slots of the test's own, with every byte outside the files checked, and the pins, computed once."""
import functools

import numpy as np

import jenc_restatement as R
import jopt_restatement as O

PATTERN, GUARD = 0xA5, 4096


@functools.lru_cache(None)
def pil(kind, w, h, index, quality):
    """PIL optimize=True of a named content, computed once per case and shared"""
    return O.pil_encode(R.to_u8(R.content(kind, w, h, index)), quality)


def encoder(w, h, quality, max_frames=1, device=0):
    from mono_dataset_code_amd import capi

    enc = capi.JpegEncoder(w, h, quality, max_frames, device=device, huffman="optimal")
    assert enc.bound == O.bound(w, h)
    return enc


def run(enc, frames, extra_stride=0, extra_slot=0, offset=0, out_offset=0):
    """One encode of `frames` (a list of h x w arrays or an (n, w * h) array; float32 or uint8 chooses the entry) -> the files.
    offset / out_offset: elements / bytes the input / output base is moved by."""
    import torch

    from mono_dataset_code_amd import capi

    host = frames if isinstance(frames, np.ndarray) and frames.ndim == 2 else np.stack([np.asarray(f).reshape(-1) for f in frames])
    assert host.dtype in (np.uint8, np.float32) and host.shape[1] == enc.w * enc.h
    n, u8 = host.shape[0], host.dtype == np.uint8
    stride, slot = enc.w * enc.h + extra_stride, enc.bound + extra_slot
    padded = np.full((n, stride), 77 if u8 else np.nan, host.dtype)
    padded[:, :enc.w * enc.h] = host
    d_in = torch.empty(n * stride + offset, dtype=torch.uint8 if u8 else torch.float32, device="cuda:0")
    d_in[offset:].copy_(torch.from_numpy(padded.reshape(-1)))
    d_out = torch.full((out_offset + n * slot + GUARD,), PATTERN, dtype=torch.uint8, device="cuda:0")
    d_sizes = torch.full((n + 16,), -77, dtype=torch.int32, device="cuda:0")
    L = capi.jopt_lib()
    fn = L.mdcjo_encode_u8_device if u8 else L.mdcjo_encode_f32_device
    rc = fn(enc._h, d_in.data_ptr() + offset * d_in.element_size(), stride, n, d_out.data_ptr() + out_offset, slot, d_sizes.data_ptr(), None)
    assert rc == 0, L.mdcjo_last_error()
    torch.cuda.synchronize()
    out, dsz = d_out.cpu().numpy(), d_sizes.cpu().numpy()
    sizes = dsz[:n].astype(np.int64)
    assert (dsz[n:] == -77).all(), "sizes written past the last frame"
    assert (sizes > 102 + 22 + 22 + 10).all() and (sizes <= enc.bound).all(), (sizes.min(), sizes.max())
    assert (out[:out_offset] == PATTERN).all() and (out[out_offset + n * slot:] == PATTERN).all(), "bytes outside the slots"
    body = out[out_offset:out_offset + n * slot].reshape(n, slot)
    if n <= 64:
        for i in range(n):
            assert (body[i, sizes[i]:] == PATTERN).all(), "slot %d written past its file" % i
    else:
        assert ((body == PATTERN) | (np.arange(slot)[None, :] < sizes[:, None])).all(), "a slot written past its file"
    return [body[i, :sizes[i]].tobytes() for i in range(n)]


def once(u8, quality, **kw):
    """one frame on an encoder of its own"""
    h, w = u8.shape
    enc = encoder(w, h, quality)
    got = run(enc, [u8], **kw)[0]
    enc.close()
    return got
