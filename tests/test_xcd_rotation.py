"""MDC_OPT_XCD_ROTATE: frame group y of a remap launch reads the placement table block -> tile shifted by y columns
(csrc/xcd_placement.h).  Placement is speed only, so with the rotation on every launch must give what it gives with the rotation
off and what the oracle gives, bit for bit: every tile of every frame group written exactly once (outputs pre-filled with -7, none
left), for tile counts 1, 2, 15, 16 (ragged last column) and 18, the four MDC_ORDER_* modes, consecutive and interleaved frame
groups, 19 groups (the rotation wraps twice), the other tile shapes, window buffers, the fused pyramid, undistort<float>, the strip
kernel (which rotates at option value 2 only) and the tapered tail."""
import os

import numpy as np
import pytest

from conftest import bits_equal, test_frames as make_frames

pytestmark = pytest.mark.gpu

FLAGS = 15  # rectify | gamma | vignette | kill overexposed
N, FPB = 38, 2  # 19 frame groups


class Cam:
    def __init__(self, folder, oracle, lines, n=N):
        from mono_dataset_code_amd import capi, synth

        d = synth.write_sequence_calibration(str(folder), lines, vignette_bits=16)
        cam = oracle.parse_camera(os.path.join(d, "camera.txt"))
        assert cam["valid"], lines
        self.W, self.H, self.w, self.h = cam["in_w"], cam["in_h"], cam["out_w"], cam["out_h"]
        self.fov = capi.UndistorterFOV(os.path.join(d, "camera.txt"))
        self.photo = capi.PhotometricUndistorter(os.path.join(d, "pcalib.txt"), os.path.join(d, "vignette.png"), self.W, self.H)
        assert self.fov.is_valid() and self.photo.valid() == 3
        self.rx, self.ry = self.fov.remap()
        self.ginv, self.vinv = self.photo.ginv(), self.photo.vignette()[1]
        self.ctx = capi.Context(0)
        self.ctx.bind(self.fov, self.photo)
        self.frames = np.stack(make_frames(self.W, self.H, n_noise=n - 3)) if n else None
        self.oracle = oracle

    def want(self, frames):
        return np.stack([self.oracle.get_image(f, self.W, self.H, self.w, self.h, self.ginv, self.vinv, True, True, self.rx, self.ry, 1, 1, 1, 1)
                         for f in frames])


def small_camera(w, h, W=320, H=240):
    return ("0.45 0.55 0.5 0.5 0.7", "%d %d" % (W, H), "crop", "%d %d" % (w, h))


# (output size, tile columns, tile rows, tiles)
SIZES = [((100, 16), 128, 16, 1), ((100, 32), 128, 16, 2), ((300, 80), 128, 16, 15), ((200, 64), 64, 16, 16), ((300, 96), 128, 16, 18)]


@pytest.mark.parametrize("size,cols,rows,tiles", SIZES, ids=["1_tile", "2_tiles", "15_tiles", "16_tiles_ragged", "18_tiles"])
def test_rotation_keeps_every_result(size, cols, rows, tiles, tmp_path, oracle):
    import torch

    from mono_dataset_code_amd import capi

    c = Cam(tmp_path, oracle, small_camera(*size))
    assert len(c.frames) == N
    ctx, st = c.ctx, torch.cuda.current_stream().cuda_stream
    ctx.set_option(capi.OPT_TWO_STAGE, 2)
    ctx.set_option(capi.OPT_KERNEL, capi.KERNEL_TILED)
    ctx.set_option(capi.OPT_TILE_COLS, cols)
    ctx.set_option(capi.OPT_TILE_ROWS, rows)
    ctx.set_option(capi.OPT_FRAMES_PER_BLOCK, FPB)
    info = ctx.info()
    assert info.tiled and (info.tile_w, info.tile_h, info.n_tiles) == (cols, rows, tiles), (info.tiled, info.tile_w, info.tile_h, info.n_tiles)
    want = c.want(c.frames)
    d_in = torch.from_numpy(c.frames).cuda()
    # undistort<float> on the same frames (its own plan, the same placement tables)
    fin = np.stack([oracle.unmap(f, c.ginv, c.vinv, True, True, 1, 1, 1) for f in c.frames])
    want_f = np.stack([oracle.undistort(x, c.rx, c.ry, c.W) for x in fin])
    d_fin = torch.from_numpy(fin).cuda()
    for order in (capi.ORDER_BANDS, capi.ORDER_ROWS, capi.ORDER_IDENTITY, capi.ORDER_BLOCKS2D):
        ctx.set_option(capi.OPT_TILE_ORDER, order)
        for il in (0, 1):
            ctx.set_option(capi.OPT_FRAME_INTERLEAVE, il)
            outs = {}
            for rot in (0, 1):
                ctx.set_option(capi.OPT_XCD_ROTATE, rot)
                d_out = torch.full((N, c.w * c.h), -7.0, dtype=torch.float32, device="cuda")
                ctx.process_batch(d_in.data_ptr(), d_out.data_ptr(), N, FLAGS, st)
                d_u = torch.full((N, c.w * c.h), -7.0, dtype=torch.float32, device="cuda")
                ctx.undistort_batch_f32(d_fin.data_ptr(), d_u.data_ptr(), N, st)
                torch.cuda.synchronize()
                outs[rot] = (d_out.cpu().numpy(), d_u.cpu().numpy())
                tag = (size, order, il, rot)
                assert not (outs[rot][0] == -7.0).any() and not (outs[rot][1] == -7.0).any(), tag
                assert bits_equal(outs[rot][0], want), tag
                assert bits_equal(outs[rot][1], want_f), tag
            assert bits_equal(outs[0][0], outs[1][0]) and bits_equal(outs[0][1], outs[1][1]), (size, order, il)


@pytest.mark.parametrize("cols,rows", [(64, 32), (128, 32)])
def test_rotation_other_tiles_window_buffers_and_fused_pyramid(cols, rows, tmp_path, oracle):
    """256 x 96 outputs are whole 64 x 32 and 128 x 32 tiles (12 and 6 of them): the four-level pyramid comes out of the same launch."""
    import torch

    from mono_dataset_code_amd import capi

    c = Cam(tmp_path, oracle, small_camera(256, 96))
    ctx, st = c.ctx, torch.cuda.current_stream().cuda_stream
    ctx.set_option(capi.OPT_TWO_STAGE, 2)
    ctx.set_option(capi.OPT_KERNEL, capi.KERNEL_TILED)
    ctx.set_option(capi.OPT_TILE_COLS, cols)
    ctx.set_option(capi.OPT_TILE_ROWS, rows)
    ctx.set_option(capi.OPT_FRAMES_PER_BLOCK, FPB)
    want = c.want(c.frames)
    lv_want = []
    for f in range(N):
        src, cw, ch, per = want[f], c.w, c.h, []
        for _ in range(3):
            src = oracle.pyramid_level(src, cw, ch)
            cw, ch = cw // 2, ch // 2
            per.append(src)
        lv_want.append(per)
    d_in = torch.from_numpy(c.frames).cuda()
    for nbuf in (2, 3):
        ctx.set_option(capi.OPT_WINDOW_BUFFERS, nbuf)
        info = ctx.info()
        assert info.tiled and (info.tile_w, info.tile_h, info.window_buffers) == (cols, rows, nbuf)
        for order, il in ((capi.ORDER_BANDS, 0), (capi.ORDER_BLOCKS2D, 1), (capi.ORDER_ROWS, 0)):
            ctx.set_option(capi.OPT_TILE_ORDER, order)
            ctx.set_option(capi.OPT_FRAME_INTERLEAVE, il)
            outs = {}
            for rot in (0, 1):
                ctx.set_option(capi.OPT_XCD_ROTATE, rot)
                d_out = torch.full((N, c.w * c.h), -7.0, dtype=torch.float32, device="cuda")
                lv = [torch.full((N, (c.w >> l) * (c.h >> l)), -7.0, dtype=torch.float32, device="cuda") for l in range(1, 4)]
                ctx.process_pyramid_batch(d_in.data_ptr(), d_out.data_ptr(), 4, [t.data_ptr() for t in lv], N, FLAGS, st)
                torch.cuda.synchronize()
                outs[rot] = [d_out.cpu().numpy()] + [t.cpu().numpy() for t in lv]
                tag = (cols, rows, nbuf, order, il, rot)
                assert all(not (o == -7.0).any() for o in outs[rot]), tag
                assert bits_equal(outs[rot][0], want), tag
                for l in range(3):
                    assert bits_equal(outs[rot][1 + l], np.stack([lv_want[f][l] for f in range(N)])), tag + (l + 1,)
            assert all(bits_equal(x, y) for x, y in zip(outs[0], outs[1])), (cols, rows, nbuf, order, il)


def test_rotation_in_the_strip_kernel(tmp_path, oracle):
    """A scale-1 rectification (512 x 240 -> 512 x 240, as the pyramid workload's camera) runs on the wave-private strip kernel: 4 x 30
    tiles of 128 x 8 in 30 groups of four waves, placed by the same tables.  The strips rotate only with the option at 2 (1, the
    default, rotates the workgroup-tiled kernels alone)."""
    import torch

    from mono_dataset_code_amd import capi, synth

    c = Cam(tmp_path, oracle, synth.camera_lines(512, 240, 512, 240))
    ctx, st = c.ctx, torch.cuda.current_stream().cuda_stream
    ctx.set_option(capi.OPT_TWO_STAGE, 1)
    ctx.set_option(capi.OPT_FRAMES_PER_BLOCK, FPB)
    assert ctx.info().two_stage and "remap_strip_kernel" in ctx.describe_launch(FLAGS, 0)
    want = c.want(c.frames)
    d_in = torch.from_numpy(c.frames).cuda()
    for order in (capi.ORDER_BANDS, capi.ORDER_ROWS, capi.ORDER_IDENTITY, capi.ORDER_BLOCKS2D):
        ctx.set_option(capi.OPT_TILE_ORDER, order)
        for il in (0, 1):
            ctx.set_option(capi.OPT_FRAME_INTERLEAVE, il)
            outs = {}
            for rot in (0, 1, 2):
                ctx.set_option(capi.OPT_XCD_ROTATE, rot)
                assert ctx.info().two_stage
                d_out = torch.full((N, c.w * c.h), -7.0, dtype=torch.float32, device="cuda")
                ctx.process_batch(d_in.data_ptr(), d_out.data_ptr(), N, FLAGS, st)
                torch.cuda.synchronize()
                outs[rot] = d_out.cpu().numpy()
                assert not (outs[rot] == -7.0).any(), (order, il, rot)
                assert bits_equal(outs[rot], want), (order, il, rot)
            assert bits_equal(outs[0], outs[1]) and bits_equal(outs[0], outs[2]), (order, il)


def test_rotation_under_the_tapered_tail(tmp_path, oracle):
    """The smallest launch whose tail is tapered (launch_tiled_variant: frames per workgroup a multiple of 8 and >= 16, at least
    4 x taper_r workgroup lengths of frames, taper_r = one resident round of workgroups in frame groups, at least 2) on 75 tiles
    of 64 x 16 -- the headline's tile count: rotation on = rotation off for every frame, sampled frames = the oracle."""
    import torch

    from mono_dataset_code_amd import capi, synth

    c = Cam(tmp_path, oracle, small_camera(320, 240), n=0)
    ctx, st = c.ctx, torch.cuda.current_stream().cuda_stream
    fpb = 16
    ctx.set_option(capi.OPT_TWO_STAGE, 2)
    ctx.set_option(capi.OPT_KERNEL, capi.KERNEL_TILED)
    ctx.set_option(capi.OPT_TILE_COLS, 64)
    ctx.set_option(capi.OPT_TILE_ROWS, 16)
    ctx.set_option(capi.OPT_WINDOW_BUFFERS, 2)
    ctx.set_option(capi.OPT_FRAMES_PER_BLOCK, fpb)
    ctx.set_option(capi.OPT_FRAME_INTERLEAVE, 0)
    ctx.set_option(capi.OPT_TAIL_TAPER, 1)
    info = ctx.info()
    assert info.tiled and (info.tile_w, info.tile_h, info.n_tiles) == (64, 16, 75)
    threads = info.tile_w * info.tile_h // 4
    resident = 256 * max(1, min(2048 // threads, 160 * 1024 // info.lds_bytes))
    n_blocks = 8 * ((info.n_tiles + 7) // 8)
    taper_r = max(2, (resident + n_blocks // 2) // n_blocks)
    n = fpb * 4 * taper_r  # the launch condition's threshold: nframes >= fpb * 4 * taper_r
    assert 64 <= n <= 4096, (n, taper_r, resident)
    npix, nout = c.W * c.H, c.w * c.h
    d_in = torch.empty(n * npix, dtype=torch.uint8, device="cuda")
    ctx.synth_frames(d_in.data_ptr(), 3, n, npix, synth.SEED, st)
    outs = {}
    for rot in (0, 1):
        ctx.set_option(capi.OPT_XCD_ROTATE, rot)
        outs[rot] = torch.full((n + 1, nout), -7.0, dtype=torch.float32, device="cuda")
        ctx.process_batch(d_in.data_ptr(), outs[rot].data_ptr(), n, FLAGS, st)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), (n, taper_r)
    assert not bool((outs[1][:n] == -7.0).any()) and bool((outs[1][n] == -7.0).all()), (n, taper_r)
    frames = d_in.view(n, npix)
    picks = [0, fpb - 1, fpb, n // 2, n - fpb // 8 - 1, n - 2, n - 1]
    want = c.want([frames[f].cpu().numpy() for f in picks])
    assert bits_equal(outs[1][picks].cpu().numpy(), want), (n, taper_r)
