"""The small frame kernels and the dispatch around them at their size and alignment edges, through the public C ABI:
unmap_scalar_kernel / unmap_xpose_kernel (unMapImage), pyramid_level_kernel, gradients_levels_kernel, remap_gather_* and
the alignment rules of enqueue_process / enqueue_undistort_f32 that choose between gather, tiled and strip kernels.

Everything is compared bit for bit (conftest.bits_equal) with the oracle and, for the box pyramid and the gradients, with the
NumPy restatements of frame_edge_problems.py as well; test_frame_edges_cpu.py shows the two equal on every case used here.
Every output lies between guard elements of -7.0 that are checked after each call.  Which case reaches which kernel:

  unmap_scalar_kernel<true/false>  npix % 4 != 0 (test_unmap_sizes: the UNMAP_SCALAR sizes), or frames at an address that is
                                   not a multiple of 4 (test_unmap_addresses: offsets 1, 2, 3); <true> with (g, v) = (1, 1)
  unmap_xpose_kernel<true/false>   npix % 4 == 0 and a 4-byte aligned base (the UNMAP_VECTOR sizes, offset 4)
  pyramid_level_kernel             mdc_pyramid_batch_device; levels 4 and 5 of the combined call; all levels without MDC_RECTIFY
  gradients_levels_kernel          mdc_gradients_batch_device (one level per launch) and the combined call (four per launch)
  remap_gather_u8 / _f32_kernel    frames at an address that is not a multiple of 16, the `ragged` camera, the synthetic remaps
"""
import numpy as np
import pytest

import frame_edge_problems as P
from conftest import bits_equal, test_frames as make_frames

pytestmark = pytest.mark.gpu

LEAD = 64  # guard elements on each side


class Out:
    """n device floats between guard elements, everything -7.0.  off4: the array starts 4 bytes past a 256-byte boundary."""

    def __init__(self, n, off4=False):
        import torch

        self.n, self.lead = int(n), LEAD + (1 if off4 else 0)
        self.t = torch.full((self.lead + self.n + LEAD,), P.GUARD, dtype=torch.float32, device="cuda")
        assert self.t.data_ptr() % 256 == 0
        self.ptr = self.t.data_ptr() + 4 * self.lead

    def get(self):
        """the array, once the guards have been seen untouched"""
        import torch

        torch.cuda.synchronize()
        a = self.t.cpu().numpy()
        assert np.all(a[:self.lead] == P.GUARD) and np.all(a[self.lead + self.n:] == P.GUARD), "guard elements were written"
        return a[self.lead:self.lead + self.n]

    def untouched(self):
        return bool(np.all(self.get() == P.GUARD))


def dev_in(arr, off=0):
    """a device copy of arr that starts `off` bytes past a 256-byte boundary -> (tensor to keep alive, address)"""
    import torch

    raw = np.ascontiguousarray(arr).view(np.uint8).ravel()
    host = np.zeros(off + raw.size + 64, np.uint8)
    host[off:off + raw.size] = raw
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 256 == 0
    return t, t.data_ptr() + off


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def flag_word(g, v, o):
    return g | (v << 1) | (o << 2)


def refused(code, call, *args):
    from mono_dataset_code_amd import capi

    with pytest.raises(capi.MdcError) as e:
        call(*args)
    assert e.value.code == code, e.value


@pytest.fixture()
def ctx():
    from mono_dataset_code_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


# ---- 2. unMapImage ----------------------------------------------------------------------------------------------------


def unmap_want(oracle, frames, ginv, vinv, g, v, o):
    want = np.stack([oracle.unmap(f, ginv, vinv, True, True, g, v, o) for f in frames])
    assert bits_equal(want, np.stack([P.unmap(f, ginv, vinv, g, v, o) for f in frames]))
    return want


@pytest.mark.parametrize("wh", P.UNMAP_SCALAR + P.UNMAP_VECTOR, ids=lambda wh: "%dpx" % (wh[0] * wh[1]))
def test_unmap_sizes(wh, ctx, oracle):
    w, h = wh
    npix, n = w * h, 5
    ginv, vinv = P.ginv_table(), P.vinv_table(npix)
    ctx.set_photometric(ginv, vinv, w, h)
    frames = P.u8_frames(npix, n, 100 + npix)
    keep, d_in = dev_in(frames)
    for g, v, o in P.unmap_flag_sets(wh):
        flags = flag_word(g, v, o)
        kernel = "%s<%s>" % ("unmap_xpose_kernel" if npix % 4 == 0 else "unmap_scalar_kernel", "true" if g and v else "false")
        assert ctx.describe_launch(flags) == kernel
        want = unmap_want(oracle, frames, ginv, vinv, g, v, o)
        out = Out(n * npix)
        ctx.unmap_batch(d_in, out.ptr, n, flags, stream())
        assert bits_equal(out.get(), want), (wh, g, v, o, "mdc_unmap_batch_device")
        out = Out(n * npix)
        ctx.process_batch(d_in, out.ptr, n, flags, stream())
        assert bits_equal(out.get(), want), (wh, g, v, o, "mdc_process_batch_device")


@pytest.mark.parametrize("wh", P.UNMAP_ADDRESS, ids=lambda wh: "%dpx" % (wh[0] * wh[1]))
def test_unmap_addresses(wh, ctx, oracle):
    """frames 1, 2, 3 bytes past a 4-byte boundary: the scalar kernel; 4 bytes past a 16-byte one: the vector kernel"""
    w, h = wh
    npix, n = w * h, 5
    ginv, vinv = P.ginv_table(), P.vinv_table(npix)
    ctx.set_photometric(ginv, vinv, w, h)
    frames = P.u8_frames(npix, n, 200 + npix)
    for g, v, o in P.ADDRESS_GVO:
        want = unmap_want(oracle, frames, ginv, vinv, g, v, o)
        for in_off, out_off4 in ((1, False), (2, False), (3, False), (4, False), (0, True), (3, True), (4, True)):
            keep, d_in = dev_in(frames, in_off)
            out = Out(n * npix, out_off4)
            ctx.unmap_batch(d_in, out.ptr, n, flag_word(g, v, o), stream())
            assert bits_equal(out.get(), want), (wh, g, v, o, in_off, out_off4)


@pytest.mark.parametrize("wh", P.UNMAP_GROUP_SIZES, ids=lambda wh: "%dpx" % (wh[0] * wh[1]))
def test_unmap_frame_groups(wh, ctx, oracle):
    """frame f's result comes from frame f's input, whatever the frames per workgroup and however short the last group"""
    from mono_dataset_code_amd import capi

    w, h = wh
    npix = w * h
    ginv, vinv = P.ginv_table(), P.vinv_table(npix)
    ctx.set_photometric(ginv, vinv, w, h)
    frames = P.u8_frames(npix, 17, 7)
    assert len({f.tobytes() for f in frames}) == 17
    want = unmap_want(oracle, frames, ginv, vinv, 1, 1, 1)
    keep, d_in = dev_in(frames)
    for fpb, n in [(0, k) for k in P.UNMAP_GROUPS_AUTO] + P.UNMAP_GROUPS_SET:
        ctx.set_option(capi.OPT_FRAMES_PER_BLOCK, fpb)
        out = Out(17 * npix)
        ctx.unmap_batch(d_in, out.ptr, n, 7, stream())
        got = out.get()
        assert bits_equal(got[:n * npix], want[:n]), (wh, fpb, n)
        assert np.all(got[n * npix:] == P.GUARD), (wh, fpb, n, "frames past nframes written")
    # no frames: nothing is written
    out = Out(17 * npix)
    ctx.unmap_batch(d_in, out.ptr, 0, 7, stream())
    ctx.process_batch(d_in, out.ptr, 0, 7, stream())
    assert out.untouched()


def test_unmap_host(ctx, oracle):
    ginv = P.ginv_table()
    for w, h in P.UNMAP_HOST:
        npix = w * h
        vinv = P.vinv_table(npix)
        ctx.set_photometric(ginv, vinv, w, h)
        for f in P.u8_frames(npix, 4, 300 + npix):
            for g, v, o in P.ALL_GVO:
                host = np.full(npix + 2 * LEAD, P.GUARD, np.float32)
                ctx.unmap_host(f, host[LEAD:LEAD + npix], flag_word(g, v, o))
                assert np.all(host[:LEAD] == P.GUARD) and np.all(host[LEAD + npix:] == P.GUARD)
                assert bits_equal(host[LEAD:LEAD + npix], oracle.unmap(f, ginv, vinv, True, True, g, v, o)), (w, h, g, v, o)


# ---- 3. stand-alone box pyramid -----------------------------------------------------------------------------------------


def pyramid_want(oracle, frames, w, h, levels):
    """per level 1 .. levels - 1 the frames' levels, oracle and restatement agreeing"""
    per_frame = [P.pyramid(f, w, h, levels, oracle.pyramid_level) for f in frames]
    for f, lv in zip(frames, per_frame):
        for a, b in zip(lv, P.pyramid(f, w, h, levels)):
            assert bits_equal(a, b)
    return [np.stack([lv[l] for lv in per_frame]) for l in range(levels - 1)]


@pytest.mark.parametrize("wh", P.PYRAMID_SIZES, ids=lambda wh: "%dx%d" % wh)
def test_pyramid_sizes(wh, ctx, oracle):
    from mono_dataset_code_amd import capi

    w, h = wh
    deepest = P.deepest(w, h)
    for n in P.PYRAMID_FRAMES:
        frames = P.f32_frames(w, h, n, 31 * w + h)
        for off4 in (False, True):
            keep, d_base = dev_in(frames, 4 if off4 else 0)
            for levels in range(1, deepest + 1) if not off4 else (deepest,):
                want = pyramid_want(oracle, frames, w, h, levels)
                outs = [Out(n * (w >> l) * (h >> l), off4) for l in range(1, levels)]
                ctx.pyramid_batch(d_base, w, h, levels, [o.ptr for o in outs], n, stream())
                for l, (o, wl) in enumerate(zip(outs, want)):
                    assert bits_equal(o.get(), wl), (wh, n, levels, l + 1, off4)
        if n == 3 and ((w & 1) or (h & 1)):  # the NaNs of the dropped column / row stayed out
            assert np.isnan(frames[2]).any() and np.isfinite(want[0][2]).all()
        # one level past the last one that is not empty: refused, nothing enqueued
        keep, d_base = dev_in(frames)
        outs = [Out(max(1, n * (w >> l) * (h >> l))) for l in range(1, deepest + 1)]
        refused(capi.ERR_ARG, ctx.pyramid_batch, d_base, w, h, deepest + 1, [o.ptr for o in outs], n, stream())
        assert all(o.untouched() for o in outs), (wh, n)
    assert (wh != (64, 64)) or deepest == 7  # the largest case reaches a 1 x 1 level


def test_empty_level_is_refused_by_every_pyramid_entry_point(ctx):
    """3 x 3 with levels = 3: level 2 would be 0 x 0.  MDC_ERR_ARG from all three calls, before anything is enqueued."""
    from mono_dataset_code_amd import capi

    w, h, n = 3, 3, 2
    ctx.set_photometric(P.ginv_table(), P.vinv_table(w * h), w, h)
    keep, d_in = dev_in(P.u8_frames(w * h, n, 1))
    keepf, d_f = dev_in(P.f32_frames(w, h, 3, 1)[:n])
    base, lv = Out(n * 9), [Out(n), Out(n)]
    dI, ab = [Out(3 * n * 9), Out(3 * n), Out(3 * n)], [Out(n * 9), Out(n), Out(n)]
    ptrs = [o.ptr for o in lv]
    refused(capi.ERR_ARG, ctx.pyramid_batch, d_f, w, h, 3, ptrs, n, stream())
    refused(capi.ERR_ARG, ctx.process_pyramid_batch, d_in, base.ptr, 3, ptrs, n, 7, stream())
    refused(capi.ERR_ARG, ctx.process_pyramid_gradients_batch, d_in, base.ptr, 3, ptrs, [o.ptr for o in dI], [o.ptr for o in ab], n, 7, 0, stream())
    assert all(o.untouched() for o in [base] + lv + dI + ab)
    # levels = 2 is the deepest: all three calls accept it
    ctx.pyramid_batch(d_f, w, h, 2, ptrs[:1], n, stream())
    ctx.process_pyramid_batch(d_in, base.ptr, 2, ptrs[:1], n, 7, stream())
    ctx.process_pyramid_gradients_batch(d_in, base.ptr, 2, ptrs[:1], [o.ptr for o in dI[:2]], [o.ptr for o in ab[:2]], n, 7, 0, stream())
    assert not base.untouched() and not lv[0].untouched() and lv[1].untouched()


# ---- 4. gradients -------------------------------------------------------------------------------------------------------


def gradients_want(oracle, frames, w, h):
    dI, ab = [], []
    for f in frames:
        (d0, a0), (d1, a1) = oracle.gradients(f, w, h), P.gradients(f, w, h)
        assert bits_equal(d0, d1) and bits_equal(a0, a1)
        dI.append(d0)
        ab.append(a0)
    return np.stack(dI), np.stack(ab)


@pytest.mark.parametrize("w", sorted({w for w, _ in P.GRAD_SIZES}))
def test_gradients_sizes(w, ctx, oracle):
    for h in [hh for ww, hh in P.GRAD_SIZES if ww == w]:
        for n in P.GRAD_FRAMES:
            frames = P.f32_frames(w, h, n, 17 * w + h)
            want_dI, want_abs = gradients_want(oracle, frames, w, h)
            for off4 in (False, True):
                keep, d_level = dev_in(frames, 4 if off4 else 0)
                dI, ab = Out(3 * n * w * h, off4), Out(n * w * h, off4)
                ctx.gradients_batch(d_level, w, h, dI.ptr, ab.ptr, n, stream())
                assert bits_equal(dI.get(), want_dI), (w, h, n, off4, "dI")
                assert bits_equal(ab.get(), want_abs), (w, h, n, off4, "absSquaredGrad")
    # no frames: nothing is written
    dI, ab = Out(3 * w), Out(w)
    ctx.gradients_batch(d_level, w, 1, dI.ptr, ab.ptr, 0, stream())
    assert dI.untouched() and ab.untouched()


@pytest.mark.parametrize("levels", P.COMBINED_LEVELS)
def test_combined_call_without_rectify(levels, ctx, oracle):
    """base, levels and gradient images of a 130 x 34 input in one call: up to four levels per gradient launch, so five and six
    levels need a second one; chunks of one and two frames leave a last chunk of one"""
    w, h = P.COMBINED_SIZE
    n = 5
    ginv, vinv = P.ginv_table(), P.vinv_table(w * h)
    ctx.set_photometric(ginv, vinv, w, h)
    frames = P.u8_frames(w * h, n, 77)
    keep, d_in = dev_in(frames)
    base = unmap_want(oracle, frames, ginv, vinv, 1, 1, 1)
    want_lv = [base] + pyramid_want(oracle, base, w, h, levels)
    want_g = [gradients_want(oracle, want_lv[l], w >> l, h >> l) for l in range(levels)]
    for chunk in P.COMBINED_CHUNKS:
        lv = [Out(n * (w >> l) * (h >> l)) for l in range(levels)]
        dI = [Out(3 * o.n) for o in lv]
        ab = [Out(o.n) for o in lv]
        ctx.process_pyramid_gradients_batch(d_in, lv[0].ptr, levels, [o.ptr for o in lv[1:]], [o.ptr for o in dI], [o.ptr for o in ab], n, 7, chunk,
                                            stream())
        for l in range(levels):
            assert bits_equal(lv[l].get(), want_lv[l]), (levels, chunk, l, "level")
            assert bits_equal(dI[l].get(), want_g[l][0]), (levels, chunk, l, "dI")
            assert bits_equal(ab[l].get(), want_g[l][1]), (levels, chunk, l, "absSquaredGrad")
    # the pyramid call without gradients writes the same levels
    lv = [Out(n * (w >> l) * (h >> l)) for l in range(levels)]
    ctx.process_pyramid_batch(d_in, lv[0].ptr, levels, [o.ptr for o in lv[1:]], n, 7, stream())
    for l in range(levels):
        assert bits_equal(lv[l].get(), want_lv[l]), (levels, l)


# ---- 5. dispatch by alignment, stores through 4-byte aligned outputs ------------------------------------------------------


class Camera:
    def __init__(self, directory, oracle):
        from mono_dataset_code_amd import capi

        self.t = t = P.camera_tables(directory)
        self.W, self.H, self.w, self.h = t["W"], t["H"], t["w"], t["h"]
        self.ctx = capi.Context(0)
        self.ctx.bind(t["fov"], t["photo"])
        self.frames = np.stack(make_frames(self.W, self.H))
        self.oracle = oracle

    def want(self, g, v, o):
        t = self.t
        return np.stack([self.oracle.get_image(f, self.W, self.H, self.w, self.h, t["ginv"], t["vinv"], True, True, t["rx"], t["ry"], 1, g, v, o)
                         for f in self.frames])


@pytest.mark.parametrize("name", P.DISPATCH_CAMERAS)
def test_process_batch_misaligned_frames(name, calib_dirs, oracle):
    """frames that do not start on a 16-byte boundary go through the gather kernel: same results as the aligned call's plan"""
    from mono_dataset_code_amd import capi

    s = Camera(calib_dirs[name], oracle)
    n, no = len(s.frames), s.w * s.h
    assert n == 5
    planned = s.ctx.describe_launch(15)
    assert planned.startswith({"small_explicit": "remap_tiled_kernel", "mag4_full_black": "remap_strip_kernel", "pyr_whole_black": "remap_tiled_kernel",
                               "ragged": "remap_gather_u8_kernel"}[name]), planned
    for flags, gvo in ((15, (1, 1, 1)), (8, (0, 0, 0))):
        want = s.want(*gvo)
        for off in (0, 1, 4, 8, 15):
            keep, d_in = dev_in(s.frames, off)
            out = Out(n * no)
            s.ctx.process_batch(d_in, out.ptr, n, flags, stream())
            assert bits_equal(out.get(), want), (name, flags, off)
    if name in P.DISPATCH_TILED:
        # the tiled kernel on request: a misaligned batch is a state error that writes nothing, and the context stays usable
        s.ctx.set_option(capi.OPT_KERNEL, capi.KERNEL_TILED)
        for off in (1, 4, 8, 15):
            keep, d_in = dev_in(s.frames, off)
            out = Out(n * no)
            refused(capi.ERR_STATE, s.ctx.process_batch, d_in, out.ptr, n, 15, stream())
            assert out.untouched(), (name, off)
        keep, d_in = dev_in(s.frames)
        out = Out(n * no)
        s.ctx.process_batch(d_in, out.ptr, n, 15, stream())
        assert bits_equal(out.get(), s.want(1, 1, 1)), name
    s.ctx.close()


@pytest.mark.parametrize("name", P.DISPATCH_CAMERAS)
def test_undistort_f32_misaligned_frames(name, calib_dirs, oracle):
    s = Camera(calib_dirs[name], oracle)
    t, no = s.t, s.w * s.h
    fin = np.stack([oracle.unmap(f, t["ginv"], t["vinv"], True, True, 1, 1, 1) for f in s.frames[:3]])
    want = np.stack([oracle.undistort(x, t["rx"], t["ry"], s.W) for x in fin])
    assert bits_equal(want, np.stack([P.bilinear(x, t["rx"], t["ry"], s.W) for x in fin]))
    for off, out_off4 in ((0, False), (4, False), (8, False), (12, False), (0, True), (4, True)):
        keep, d_in = dev_in(fin, off)
        out = Out(3 * no, out_off4)
        s.ctx.undistort_batch_f32(d_in, out.ptr, 3, stream())
        assert bits_equal(out.get(), want), (name, off, out_off4)
    s.ctx.close()


@pytest.mark.parametrize("name", P.DISPATCH_TILED)
def test_outputs_on_4_byte_boundaries(name, calib_dirs, oracle):
    """aligned frames, so the tiled / strip / fused-pyramid kernels run; base and levels start 4 bytes past a 256-byte boundary"""
    from mono_dataset_code_amd import capi

    s = Camera(calib_dirs[name], oracle)
    n, no, levels = len(s.frames), s.w * s.h, 4
    want = s.want(1, 1, 1)
    want_lv = pyramid_want(oracle, want, s.w, s.h, levels)
    keep, d_in = dev_in(s.frames)
    out = Out(n * no, True)
    s.ctx.process_batch(d_in, out.ptr, n, 15, stream())
    assert bits_equal(out.get(), want), name
    # the plan as chosen, and for the camera made of whole 64 x 32 tiles those tiles: levels 1..3 out of the remap launch
    for cols, rows in ((0, 0), (64, 32)) if name == "pyr_whole_black" else ((0, 0),):
        s.ctx.set_option(capi.OPT_TILE_COLS, cols)
        s.ctx.set_option(capi.OPT_TILE_ROWS, rows)
        kernel = s.ctx.describe_launch(15, levels)
        if rows:
            assert kernel.startswith("remap_tiled_kernel<true, true, true, false, 64, %d" % (16 * rows)), kernel
        if name == "mag4_full_black":
            assert kernel.startswith("remap_strip_kernel<true, true"), kernel
        for off4 in (False, True):
            base = Out(n * no, off4)
            lv = [Out(n * (s.w >> l) * (s.h >> l), off4) for l in range(1, levels)]
            s.ctx.process_pyramid_batch(d_in, base.ptr, levels, [o.ptr for o in lv], n, 15, stream())
            assert bits_equal(base.get(), want), (name, kernel, off4)
            for l in range(levels - 1):
                assert bits_equal(lv[l].get(), want_lv[l]), (name, kernel, off4, l + 1)
    s.ctx.close()


@pytest.mark.parametrize("geom", P.SYNTH_REMAPS, ids=lambda g: "%dx%d_to_%dx%d" % g)
def test_gather_below_one_workgroup(geom, ctx, oracle):
    iw, ih, ow, oh = geom
    n = 5
    rx, ry = P.remap_tables(iw, ih, ow, oh, 5)
    ginv, vinv = P.ginv_table(), P.vinv_table(iw * ih)
    ctx.set_photometric(ginv, vinv, iw, ih)
    ctx.set_remap(rx, ry, iw, ih, ow, oh)
    assert ctx.describe_launch(15) == "remap_gather_u8_kernel<true>" and ctx.describe_launch(8) == "remap_gather_u8_kernel<false>"
    assert ctx.describe_launch(0, -1) == "remap_gather_f32_kernel"
    frames = P.u8_frames(iw * ih, n, 9)
    keep, d_in = dev_in(frames)
    for flags, (g, v, o) in ((15, (1, 1, 1)), (8, (0, 0, 0))):
        want = np.stack([oracle.get_image(f, iw, ih, ow, oh, ginv, vinv, True, True, rx, ry, 1, g, v, o) for f in frames])
        assert bits_equal(want, np.stack([P.bilinear(P.unmap(f, ginv, vinv, g, v, o), rx, ry, iw) for f in frames]))
        out = Out(n * ow * oh)
        ctx.process_batch(d_in, out.ptr, n, flags, stream())
        assert bits_equal(out.get(), want), (geom, flags)
    fin = np.stack([oracle.unmap(f, ginv, vinv, True, True, 1, 1, 1) for f in frames])
    keepf, d_f = dev_in(fin)
    out = Out(n * ow * oh)
    ctx.undistort_batch_f32(d_f, out.ptr, n, stream())
    assert bits_equal(out.get(), np.stack([oracle.undistort(x, rx, ry, iw) for x in fin])), geom


# ---- 6. more frame groups than 65,535 ---------------------------------------------------------------------------------------


def test_more_frame_groups_than_grid_rows(ctx, oracle):
    """65,537 frames of 8 x 8 at one frame per workgroup: grids of (1, 65537).  The other libraries here treat 65,535 as the rows a
    launch grid may have; launch_unmap and launch_remap_gather_* put every frame group into one grid, and the runtime takes it.
    Frame f holds content f % 13 and must come out as that content's result."""
    from mono_dataset_code_amd import capi

    w = h = 8
    n, npix = P.MANY_GROUPS, 64
    ginv, vinv = P.ginv_table(), P.vinv_table(npix)
    rx, ry = P.remap_tables(w, h, w, h, 5)
    ctx.set_photometric(ginv, vinv, w, h)
    ctx.set_remap(rx, ry, w, h, w, h)
    ctx.set_option(capi.OPT_FRAMES_PER_BLOCK, 1)
    assert ctx.describe_launch(15) == "remap_gather_u8_kernel<true>"
    kinds = P.u8_frames(npix, 13, 9)
    assert len({k.tobytes() for k in kinds}) == 13
    which = np.arange(n) % 13
    keep, d_in = dev_in(kinds[which])
    want = np.stack([oracle.unmap(k, ginv, vinv, True, True, 1, 1, 1) for k in kinds])
    out = Out(n * npix)
    ctx.unmap_batch(d_in, out.ptr, n, 7, stream())
    assert bits_equal(out.get(), want[which]), "mdc_unmap_batch_device"
    want = np.stack([oracle.get_image(k, w, h, w, h, ginv, vinv, True, True, rx, ry, 1, 1, 1, 1) for k in kinds])
    out = Out(n * npix)
    ctx.process_batch(d_in, out.ptr, n, 15, stream())
    assert bits_equal(out.get(), want[which]), "mdc_process_batch_device"
    fin = np.stack([oracle.unmap(k, ginv, vinv, True, True, 1, 1, 0) for k in kinds])
    keepf, d_f = dev_in(fin[which])
    want = np.stack([oracle.undistort(x, rx, ry, w) for x in fin])
    out = Out(n * npix)
    ctx.undistort_batch_f32(d_f, out.ptr, n, stream())
    assert bits_equal(out.get(), want[which]), "mdc_undistort_batch_device_f32"
