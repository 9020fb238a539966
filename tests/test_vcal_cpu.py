"""The facts tests/test_vcal_sizes.py builds on, checked without a GPU:

- compaction: the plane step and the vignette step skip a sample with a NaN coordinate before any arithmetic and keep images in
  order and, within an image, plane points in ascending order.  So a problem whose only valid samples are a few (image, plane
  point) pairs gives, bit for bit, what the compacted problem (those images and points only) gives -- E too, a sequential sum
  over the same terms.  That is what lets the GPU tests build stacks past 2^31 elements sparsely and run the oracle on the
  compacted arrays.
- the listed-sample count (vcal_problems.listed), which the GPU tests assert the index's entry count against exactly, is the
  oracle's R of a first plane step with every factor 1, every plane colour 0 and no outlier."""
import numpy as np

import vcal_problems as P
from conftest import bits_equal

SENTINEL = np.float32(1e30)


def sparse_problem(seed):
    """9 images of 23 x 17, 300 plane points; images 1, 4 and 7 and a third of the plane points have no coordinate at all and
    the images without coordinates hold a sentinel; a few NaN pixels and NaN samples inside the rest."""
    rng = np.random.default_rng(seed)
    n, w, h, npt = 9, 23, 17, 300
    images = (40 + 50 * rng.random((n, h, w))).astype(np.float32)
    images[rng.random((n, h, w)) < 0.03] = np.nan
    p2x = rng.uniform(0, w - 1, (n, npt)).astype(np.float32)
    p2y = rng.uniform(0, h - 1, (n, npt)).astype(np.float32)
    np.minimum(p2x, np.nextafter(np.float32(w - 1), np.float32(0)), out=p2x)
    np.minimum(p2y, np.nextafter(np.float32(h - 1), np.float32(0)), out=p2y)
    dead_imgs = np.array([1, 4, 7])
    dead_pts = np.sort(rng.choice(npt, npt // 3, replace=False))
    dead_pts = np.union1d(dead_pts, [0, npt - 1])
    images[dead_imgs] = SENTINEL
    p2x[dead_imgs] = np.nan
    p2x[:, dead_pts] = np.nan
    p2x[rng.random((n, npt)) < 0.05] = np.nan
    p2y[np.isnan(p2x)] = np.nan
    imgs = np.setdiff1d(np.arange(n), dead_imgs)
    pts = np.setdiff1d(np.arange(npt), dead_pts)
    return images, p2x, p2y, imgs, pts


def alternate(step_plane, step_vig, images, p2x, p2y, iters=4):
    """iters alternating half-iterations from planeColor 0, vignetteFactor 1, 2 each side of the outlier switch"""
    n, h, w = images.shape
    pc = np.zeros(p2x.shape[1], np.float32)
    vf = np.ones(h * w, np.float32)
    out = []
    for it in range(iters):
        oth2 = 10000 * 10000 if it < iters // 2 else 15 * 15
        pc, ff, fc, e1, r1 = step_plane(images, p2x, p2y, pc, vf, oth2)
        vf, tt, ct, e2, r2 = step_vig(images, p2x, p2y, pc, vf, oth2)
        out.append(dict(pc=pc, ff=ff, fc=fc, e1=e1, r1=r1, vf=vf, tt=tt, ct=ct, e2=e2, r2=r2))
    return out


def assert_compaction(full, comp, pts):
    dead = np.setdiff1d(np.arange(full[0]["pc"].size), pts)
    for it, (a, b) in enumerate(zip(full, comp)):
        for key in ("pc", "ff", "fc"):
            assert bits_equal(a[key][pts], b[key]), (it, key)
        assert not np.any(a["ff"][dead]) and not np.any(a["fc"][dead]) and np.isnan(a["pc"][dead]).all(), it
        for key in ("vf", "tt", "ct"):
            assert bits_equal(a[key], b[key]), (it, key)
        for key in ("e1", "r1", "e2", "r2"):
            assert a[key] == b[key], (it, key)
    assert full[-1]["r2"] > 100 and np.isfinite(full[-1]["vf"]).sum() > 50


def test_compaction_invariance_oracle(oracle):
    for seed in range(3):
        images, p2x, p2y, imgs, pts = sparse_problem(seed)
        full = alternate(oracle.vcal_plane_step, oracle.vcal_vignette_step, images, p2x, p2y)
        comp = alternate(oracle.vcal_plane_step, oracle.vcal_vignette_step, *P.compact(images, p2x, p2y, imgs, pts))
        assert_compaction(full, comp, pts)


def test_compaction_invariance_reference_loops(oracle):
    """the same with the reference's own loop text, where it was built here (oracle/_ref/libvcal_ref.so), and the oracle's
    answer for the compacted problem equals it"""
    from oracle import loader

    try:
        live = loader.VcalRef()
    except OSError:
        live = None
    for seed in range(3 if live else 0):
        images, p2x, p2y, imgs, pts = sparse_problem(seed)

        def plane(im, x, y, pc, vf, oth2):
            return live.plane_step(im, x, y, x.shape[1], 1, pc, vf, oth2)

        def vig(im, x, y, pc, vf, oth2):
            return live.vignette_step(im, x, y, x.shape[1], 1, pc, vf, oth2)

        full = alternate(plane, vig, images, p2x, p2y)
        small = P.compact(images, p2x, p2y, imgs, pts)
        comp = alternate(plane, vig, *small)
        assert_compaction(full, comp, pts)
        ours = alternate(oracle.vcal_plane_step, oracle.vcal_vignette_step, *small)
        assert_compaction(full, ours, pts)


def test_listed_count_is_the_first_plane_steps_R(oracle):
    """vcal_problems.listed over NaN coordinates, NaN pixels at each of the four taps, sentinel images and samples on the last
    admissible row and column = R of a plane step with factors 1, colours 0 and oth2 = 10^8 (every sample counted once)"""
    rng = np.random.default_rng(17)
    for n, w, h in ((5, 31, 19), (3, 2, 2), (4, 2, 9), (4, 40, 2)):
        images = (rng.random((n, h, w)) * 200).astype(np.float32)
        images[rng.random((n, h, w)) < 0.08] = np.nan
        npt = 400
        p2x = rng.uniform(0, w - 1, (n, npt)).astype(np.float32)
        p2y = rng.uniform(0, h - 1, (n, npt)).astype(np.float32)
        p2x[:, :3] = np.nextafter(np.float32(w - 1), np.float32(0))
        p2y[:, 3:6] = np.nextafter(np.float32(h - 1), np.float32(0))
        p2x[:, 6], p2y[:, 7] = np.float32(-0.0), np.float32(0.0)
        np.minimum(p2x, np.nextafter(np.float32(w - 1), np.float32(0)), out=p2x)
        np.minimum(p2y, np.nextafter(np.float32(h - 1), np.float32(0)), out=p2y)
        p2x[rng.random((n, npt)) < 0.1] = np.nan
        p2y[np.isnan(p2x)] = np.nan
        if n > 3:
            images[1] = SENTINEL
        mask, b = P.listed(images, p2x, p2y)
        assert mask.sum() == b.size and 0 < b.size < mask.size
        _, _, _, e, r = oracle.vcal_plane_step(images, p2x, p2y, np.zeros(npt, np.float32), np.ones(w * h, np.float32), 10 ** 8)
        assert r == b.size, (n, w, h)
        # the entries of the index, per bin, sum to 4 per listed sample
        assert P.bin_counts(b, w, h).sum() == 4 * b.size
