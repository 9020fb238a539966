"""Sizes, synthetic tables and plain NumPy restatements for the frame kernels' edge tests (test_frame_edges_cpu.py on the CPU,
test_frame_edges.py on the GPU).

The restatements are written from the definitions -- include/mdc_hip.h, DESIGN.md section 5.5, the reference's expression order as
oracle/mdc_oracle.c quotes it -- in float32 operations, one NumPy expression per C operation, and from nothing in the kernels.
The case lists are the sizes at which the kernels' loops, lanes and launch rules change:

  unmap_xpose_kernel        a workgroup owns 4096 pixels: four runs of 1024 per wave set, 256 per wave, 64 per store
  unmap_scalar_kernel       taken when npix % 4 != 0 or the frames' base is not 4-byte aligned; 256 pixels per workgroup
  pyramid_level_kernel      one output per thread; source pitch w, output pitch w >> 1
  gradients_levels_kernel   waves of 64 columns, workgroups of 128, bands of 8 rows; lanes 0 and nvalid - 1 load their own neighbours
  remap_gather_*            taken when no tile / strip plan exists or the frames' base is not 16-byte aligned
"""
import numpy as np

F32 = np.float32
GUARD = -7.0

# ---- synthetic tables -------------------------------------------------------------------------------------------------


def ginv_table():
    """strictly increasing, no entry an integer"""
    g = (np.arange(256, dtype=np.float64) * 1.03125 + 0.37).astype(F32)
    assert np.all(np.diff(g) > 0) and not np.any(g == np.floor(g))
    return g


def vinv_table(n):
    """distinct over any 251 neighbouring pixels, exact in float32"""
    return (F32(1) + (np.arange(n) % 251).astype(F32) / F32(256)).astype(F32)


def remap_tables(in_w, in_h, out_w, out_h, seed):
    """taps strictly inside (0, in_w - 1) x (0, in_h - 1) with varying fractional parts; about one entry in eleven (-1, -1)"""
    rng = np.random.default_rng(seed)
    n = out_w * out_h
    rx = rng.uniform(0.05, in_w - 1.05, n).astype(F32)
    ry = rng.uniform(0.05, in_h - 1.05, n).astype(F32)
    black = np.arange(n) % 11 == 5
    rx[black] = -1
    ry[black] = -1
    ok = ~black
    assert np.all((rx[ok] > 0) & (rx[ok] < in_w - 1) & (ry[ok] > 0) & (ry[ok] < in_h - 1))
    return rx, ry


# ---- inputs -----------------------------------------------------------------------------------------------------------


def u8_frames(npix, nframes, seed):
    """frame 0 noise, 1 all 255, 2 all 0, 3 the ramp i % 256, then noise: every frame differs from the others (npix >= 4)"""
    rng = np.random.default_rng(seed)
    out = np.empty((nframes, npix), np.uint8)
    for f in range(nframes):
        if f == 1:
            out[f] = 255
        elif f == 2:
            out[f] = 0
        elif f == 3:
            out[f] = np.arange(npix) % 256
        else:
            out[f] = rng.integers(0, 256, npix, dtype=np.uint8)
            if npix >= 8:
                out[f, :: max(7, npix // 5)] = 255  # overexposed pixels inside the noise
                out[f, 0] = (17 * f + 3) % 251  # and the frame number where a mix-up of frames shows
    return out


def f32_noise(w, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0, 255, w * h).astype(F32) * F32(1.0078125)).astype(F32)


_SPECIAL = (np.nan, np.inf, -np.inf)


def special_positions(w, h):
    """(x, y) where the float frames carry NaN / +inf / -inf: corners, first / last row and column, an interior pixel, the columns
    on both sides of every 64-column wave boundary (the neighbours the first and the last lane of a wave load themselves), and
    column w - 1 where w % 64 == 1 (one lane is both)."""
    pos = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2), (w // 3, h // 2)]
    row = 0
    for c in range(64, w, 64):
        pos.append((c - 1, 1 if h == 3 else (row + 1) % h))
        pos.append((c, 1 if h == 3 else (2 * row + 2) % h))  # h = 3: row 1 is the only row with differences
        if h > 4:
            pos.append((c - 1, h - 2))
            pos.append((c, h // 2 + 1))
        row += 1
    if w % 64 == 1:
        pos += [(w - 1, y) for y in range(1, h, 3)]
    seen, out = set(), []
    for p in pos:
        if p not in seen:
            seen.add(p)
            out.append(p)
    return out


def f32_special(w, h, seed, shift=0):
    a = f32_noise(w, h, seed)
    for k, (x, y) in enumerate(special_positions(w, h)):
        a[y * w + x] = _SPECIAL[(k + shift) % 3]
    return a


def f32_dropped(w, h, seed):
    """NaN exactly where a box level of an odd size drops its source: the last column of an odd w, the last row of an odd h"""
    a = f32_noise(w, h, seed).reshape(h, w)
    if w & 1:
        a[:, w - 1] = np.nan
    if h & 1:
        a[h - 1, :] = np.nan
    return a.ravel()


def f32_frames(w, h, nframes, seed):
    """nframes = 1: the frame with the special values; 3: noise, special values, NaN in the dropped column / row"""
    if nframes == 1:
        return f32_special(w, h, seed)[None]
    return np.stack([f32_noise(w, h, seed + 1), f32_special(w, h, seed + 2, 1), f32_dropped(w, h, seed + 3)] +
                    [f32_special(w, h, seed + 4 + k, k) for k in range(nframes - 3)])


# ---- restatements -----------------------------------------------------------------------------------------------------


def unmap(raw_u8, ginv, vinv, g, v, o):
    """PhotometricUndistorter::unMapImage with both tables valid: the vignette needs the response (v without g = neither);
    B = Ginv[raw] or raw; overexposed pixels (255) -> NaN when asked; then * vinv."""
    raw = np.asarray(raw_u8, np.uint8).ravel()
    if v and not g:
        g = v = 0
    out = ginv.astype(F32)[raw] if g else raw.astype(F32)
    if v:
        out = (out * vinv.astype(F32)).astype(F32)
    if o:
        out = out.copy()
        out[raw == 255] = np.nan
    return out.astype(F32)


def box_level(src, w, h):
    """0.25f * (((a + b) + c) + d) over (w >> 1) x (h >> 1), source pitch w"""
    s = np.asarray(src, F32).reshape(h, w)
    w2, h2 = w >> 1, h >> 1
    a, b = s[0:2 * h2:2, 0:2 * w2:2], s[0:2 * h2:2, 1:2 * w2:2]
    c, d = s[1:2 * h2:2, 0:2 * w2:2], s[1:2 * h2:2, 1:2 * w2:2]
    with np.errstate(all="ignore"):
        return (F32(0.25) * (((a + b) + c) + d)).astype(F32).ravel()


def gradients(I, w, h):
    """-> dI (w * h, 3) = (I, dx, dy), abs (w * h): central differences over the LINEAR index range [w, w * (h - 1)), non-finite
    differences 0, everything outside the range 0"""
    I = np.asarray(I, F32).ravel()
    n = w * h
    dI, a = np.zeros((n, 3), F32), np.zeros(n, F32)
    dI[:, 0] = I
    if w * (h - 1) > w:
        i = np.arange(w, w * (h - 1))
        with np.errstate(all="ignore"):
            dx = (F32(0.5) * (I[i + 1] - I[i - 1])).astype(F32)
            dy = (F32(0.5) * (I[i + w] - I[i - w])).astype(F32)
            dx[~np.isfinite(dx)] = 0
            dy[~np.isfinite(dy)] = 0
            dI[i, 1], dI[i, 2] = dx, dy
            a[i] = (dx * dx + dy * dy).astype(F32)
    return dI, a


def bilinear(img, rx, ry, in_w):
    """UndistorterFOV::undistort: xxyy * src[1 + W] + (yy - xxyy) * src[W] + (xx - xxyy) * src[1] + (1 - xx - yy + xxyy) * src[0],
    left to right; (-1, -1) -> 0"""
    src = np.asarray(img).ravel().astype(F32)
    rx, ry = np.asarray(rx, F32), np.asarray(ry, F32)
    black = rx < 0
    xx, yy = np.where(black, F32(0), rx).astype(F32), np.where(black, F32(0), ry).astype(F32)
    xi, yi = xx.astype(np.int32), yy.astype(np.int32)
    xx, yy = (xx - xi.astype(F32)).astype(F32), (yy - yi.astype(F32)).astype(F32)
    s = xi + yi * in_w
    s = np.where(black, 0, s)
    with np.errstate(all="ignore"):
        xxyy = (xx * yy).astype(F32)
        r = ((xxyy * src[s + 1 + in_w] + (yy - xxyy) * src[s + in_w]) + (xx - xxyy) * src[s + 1]) + (((F32(1) - xx) - yy) + xxyy) * src[s]
    return np.where(black, F32(0), r).astype(F32)


def pyramid(base, w, h, levels, level=box_level):
    """levels 1 .. levels - 1 of one frame"""
    out, src = [], base
    for l in range(1, levels):
        src = level(src, w >> (l - 1), h >> (l - 1))
        out.append(src)
    return out


def deepest(w, h):
    """the largest `levels` whose last level is still at least 1 x 1"""
    n = 1
    while (w >> n) >= 1 and (h >> n) >= 1:
        n += 1
    return n


# ---- case lists -------------------------------------------------------------------------------------------------------

ALL_GVO = [(g, v, o) for g in (0, 1) for v in (0, 1) for o in (0, 1)]
TWO_GVO = [(1, 1, 1), (0, 0, 1)]

# unMapImage, scalar path by size (npix % 4 != 0): npix -> (w, h)
UNMAP_SCALAR = [(1, 1), (2, 1), (3, 1), (5, 1), (7, 5), (51, 5), (257, 1), (65, 63), (17, 241), (8191, 1)]
# unMapImage, vector path: +-4 pixels around one store (64), one wave's run (256), one wave set (1024), one workgroup (4096)
UNMAP_VECTOR = [(2, 2), (10, 6), (8, 8), (17, 4), (18, 14), (16, 16), (20, 13), (34, 30), (32, 32), (257, 4), (62, 66), (64, 64),
                (82, 50), (89, 92), (128, 64), (12, 683), (28, 439)]
UNMAP_ALL_FLAGS = [(7, 5), (257, 1), (17, 241), (62, 66), (82, 50)]  # 35, 257, 4097 scalar; 4092, 4100 vector
assert sorted(w * h for w, h in UNMAP_SCALAR) == [1, 2, 3, 5, 35, 255, 257, 4095, 4097, 8191]
assert sorted(w * h for w, h in UNMAP_VECTOR) == [4, 60, 64, 68, 252, 256, 260, 1020, 1024, 1028, 4092, 4096, 4100, 8188, 8192, 8196, 12292]
UNMAP_ADDRESS = [(64, 64), (82, 50)]  # 4096, 4100
ADDRESS_GVO = [(1, 1, 1), (1, 0, 0), (0, 0, 1)]  # both VIG instantiations
UNMAP_GROUPS_AUTO =[1, 7, 8, 9, 16, 17]  # nframes with MDC_OPT_FRAMES_PER_BLOCK 0 (the rule caps at 8 frames per group)
UNMAP_GROUPS_SET = [(1, 7), (3, 7), (5, 7), (3, 17), (5, 16)]  # (frames per group, nframes)
UNMAP_GROUP_SIZES = [(20, 13), (257, 1)]  # 260 pixels: vector path; 257: scalar path
UNMAP_HOST = [(7, 5), (17, 241), (82, 50)]


def unmap_flag_sets(wh):
    return ALL_GVO if wh in UNMAP_ALL_FLAGS else TWO_GVO


PYRAMID_SIZES = [(2, 2), (3, 2), (2, 3), (3, 3), (5, 7), (255, 3), (257, 2), (513, 5), (33, 31), (64, 64)]
PYRAMID_FRAMES = [1, 3]

GRAD_SIZES = [(w, h) for w in (1, 2, 3, 63, 64, 65, 127, 128, 129, 257) for h in (1, 2, 3)] + [(w, h) for w in (1, 65, 129) for h in (7, 8, 9, 17)]
GRAD_FRAMES = [1, 3]
COMBINED_SIZE = (130, 34)
COMBINED_LEVELS = [1, 4, 5, 6]
COMBINED_CHUNKS = [0, 1, 2]

DISPATCH_CAMERAS = ["small_explicit", "mag4_full_black", "pyr_whole_black", "ragged"]
DISPATCH_TILED = ["small_explicit", "mag4_full_black", "pyr_whole_black"]
SYNTH_REMAPS = [(7, 5, 9, 3), (2, 2, 1, 1)]

MANY_GROUPS = 65537  # frame groups of one frame each: one more than 65,536, two more than the grid rows other launchers here allow


def camera_tables(directory):
    """(W, H, w, h, rx, ry, ginv, vinv) of a calib_dirs camera, from the product's host classes (no GPU needed); the objects too"""
    import os

    from mono_dataset_code_amd import capi

    fov = capi.UndistorterFOV(os.path.join(directory, "camera.txt"))
    assert fov.is_valid()
    W, H, w, h = fov.dims()
    photo = capi.PhotometricUndistorter(os.path.join(directory, "pcalib.txt"), os.path.join(directory, "vignette.png"), W, H)
    assert photo.valid() == 3
    rx, ry = fov.remap()
    return {"W": W, "H": H, "w": w, "h": h, "rx": rx, "ry": ry, "ginv": photo.ginv(), "vinv": photo.vignette()[1], "fov": fov, "photo": photo}
