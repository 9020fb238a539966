"""The NumPy restatements of frame_edge_problems.py against the oracle, bit for bit, on every size and input that
test_frame_edges.py gives the device.  oracle.unmap and oracle.undistort are pinned to the reference build by
test_oracle_vs_ref.py; for pyramid_level and gradients, which the reference does not have, this is a second statement of the
project's own definition, written independently of the oracle's C text and of the kernels.  No GPU."""
import numpy as np

import frame_edge_problems as P
from conftest import bits_equal, test_frames as make_frames


def test_tables_are_what_the_tests_need():
    g = P.ginv_table()
    assert g.dtype == np.float32 and np.all(np.diff(g) > 0) and not np.any(g == np.floor(g))
    v = P.vinv_table(12292)
    assert len(set(v[:251].tolist())) == 251 and np.all(v >= 1) and np.all(v < 2)
    for iw, ih, ow, oh in P.SYNTH_REMAPS + [(8, 8, 8, 8)]:
        rx, ry = P.remap_tables(iw, ih, ow, oh, 5)
        assert rx.size == ow * oh and np.array_equal(rx < 0, ry < 0)
    rx, _ = P.remap_tables(8, 8, 8, 8, 5)
    assert 3 <= int((rx < 0).sum()) <= 8
    fr = P.u8_frames(260, 17, 1)
    assert len({f.tobytes() for f in fr}) == 17  # every frame differs
    for w, h in P.GRAD_SIZES + P.PYRAMID_SIZES:
        sp = P.f32_special(w, h, 1)
        assert np.isnan(sp).any() or w * h < 3
        if w > 64:
            assert not np.isfinite(sp.reshape(h, w)[:, 63]).all() and not np.isfinite(sp.reshape(h, w)[:, 64]).all()
        if w % 64 == 1 and h > 1:
            assert not np.isfinite(sp.reshape(h, w)[1:, w - 1]).all()


def test_unmap_restatement_equals_oracle(oracle):
    ginv = P.ginv_table()
    cases = 0
    for w, h in P.UNMAP_SCALAR + P.UNMAP_VECTOR:
        vinv = P.vinv_table(w * h)
        for f in P.u8_frames(w * h, 5, 100 + w * h):
            for g, v, o in P.unmap_flag_sets((w, h)):
                assert bits_equal(P.unmap(f, ginv, vinv, g, v, o), oracle.unmap(f, ginv, vinv, True, True, g, v, o)), (w, h, g, v, o)
                cases += 1
    for w, h in P.UNMAP_GROUP_SIZES:
        vinv = P.vinv_table(w * h)
        for f in P.u8_frames(w * h, 17, 7):
            assert bits_equal(P.unmap(f, ginv, vinv, 1, 1, 1), oracle.unmap(f, ginv, vinv, True, True, 1, 1, 1))
            cases += 1
    for w, h in P.UNMAP_ADDRESS:  # the frames of the address cases
        vinv = P.vinv_table(w * h)
        for f in P.u8_frames(w * h, 5, 200 + w * h):
            for g, v, o in P.ADDRESS_GVO:
                assert bits_equal(P.unmap(f, ginv, vinv, g, v, o), oracle.unmap(f, ginv, vinv, True, True, g, v, o)), (w, h, g, v, o)
                cases += 1
    for w, h in P.UNMAP_HOST:  # the frames of mdc_unmap_host
        vinv = P.vinv_table(w * h)
        for f in P.u8_frames(w * h, 4, 300 + w * h):
            for g, v, o in P.ALL_GVO:
                assert bits_equal(P.unmap(f, ginv, vinv, g, v, o), oracle.unmap(f, ginv, vinv, True, True, g, v, o)), (w, h, g, v, o)
                cases += 1
    for f in P.u8_frames(64, 13, 9):  # the 65,537-frame batch holds these thirteen
        assert bits_equal(P.unmap(f, ginv, P.vinv_table(64), 1, 1, 1), oracle.unmap(f, ginv, P.vinv_table(64), True, True, 1, 1, 1))
        cases += 1
    print("section 2 (unMapImage): %d frame x flag cases" % cases)
    assert cases == (5 * 8 + 22 * 2) * 5 + 2 * 17 + 13 + 2 * 5 * 3 + 3 * 4 * 8


def test_box_level_restatement_equals_oracle(oracle):
    cases = 0
    for w, h in P.PYRAMID_SIZES:
        for n in P.PYRAMID_FRAMES:
            for f in P.f32_frames(w, h, n, 31 * w + h):
                mine, theirs = P.pyramid(f, w, h, P.deepest(w, h)), P.pyramid(f, w, h, P.deepest(w, h), oracle.pyramid_level)
                assert len(mine) == P.deepest(w, h) - 1 >= 1
                for l, (a, b) in enumerate(zip(mine, theirs)):
                    assert a.size == ((w >> (l + 1)) * (h >> (l + 1))) and bits_equal(a, b), (w, h, n, l + 1)
                    cases += 1
        # NaN only in the column / row an odd size drops: nothing of it in any level
        if (w & 1) or (h & 1):
            assert np.isnan(P.f32_dropped(w, h, 3)).any()
            assert all(np.isfinite(a).all() for a in P.pyramid(P.f32_dropped(w, h, 3), w, h, 2))
    assert P.deepest(64, 64) == 7 and P.deepest(3, 3) == 2 and P.deepest(513, 5) == 3
    print("section 3 (box pyramid): %d frame x level cases" % cases)
    assert cases == 4 * sum(P.deepest(w, h) - 1 for w, h in P.PYRAMID_SIZES)


def test_gradients_restatement_equals_oracle(oracle):
    cases = 0
    for w, h in P.GRAD_SIZES:
        for n in P.GRAD_FRAMES:
            for f in P.f32_frames(w, h, n, 17 * w + h):
                (d0, a0), (d1, a1) = P.gradients(f, w, h), oracle.gradients(f, w, h)
                assert bits_equal(d0, d1) and bits_equal(a0, a1), (w, h, n)
                assert not np.isnan(a0).any() and not np.isnan(d0[:, 1:]).any()
                if h <= 2:
                    assert not d0[:, 1:].any() and not a0.any()
                cases += 1
    assert len(P.GRAD_SIZES) == 42
    # w = 1 follows the linear index: dx and dy are the same difference
    d, _ = P.gradients(np.arange(9, dtype=np.float32) ** 2, 1, 9)
    assert np.array_equal(d[:, 1], d[:, 2]) and d[4, 1] == 0.5 * (25 - 9)
    print("section 4 (gradients): %d frames" % cases)
    assert cases == 42 * 4


def test_combined_call_restatement_equals_oracle(oracle):
    w, h = P.COMBINED_SIZE
    ginv, vinv = P.ginv_table(), P.vinv_table(w * h)
    cases = 0
    for f in P.u8_frames(w * h, 5, 77):
        b0, b1 = P.unmap(f, ginv, vinv, 1, 1, 1), oracle.unmap(f, ginv, vinv, True, True, 1, 1, 1)
        assert bits_equal(b0, b1)
        lv0, lv1 = [b0] + P.pyramid(b0, w, h, 6), [b1] + P.pyramid(b1, w, h, 6, oracle.pyramid_level)
        for l in range(6):
            (d0, a0), (d1, a1) = P.gradients(lv0[l], w >> l, h >> l), oracle.gradients(lv1[l], w >> l, h >> l)
            assert bits_equal(lv0[l], lv1[l]) and bits_equal(d0, d1) and bits_equal(a0, a1), l
            cases += 1
    assert P.deepest(w, h) == 6
    print("section 4 (combined call): %d frame x level cases" % cases)
    assert cases == 30


def test_bilinear_restatement_equals_oracle(oracle, calib_dirs):
    cases = 0
    for name in P.DISPATCH_CAMERAS:
        t = P.camera_tables(calib_dirs[name])
        for f in make_frames(t["W"], t["H"]):
            for g, v, o in ((1, 1, 1), (0, 0, 0)):  # flags 15 and 8
                want = oracle.get_image(f, t["W"], t["H"], t["w"], t["h"], t["ginv"], t["vinv"], True, True, t["rx"], t["ry"], 1, g, v, o)
                un = P.unmap(f, t["ginv"], t["vinv"], g, v, o)
                assert bits_equal(P.bilinear(un, t["rx"], t["ry"], t["W"]), want), (name, g, v, o)
                assert bits_equal(oracle.undistort(un, t["rx"], t["ry"], t["W"]), want), (name, g, v, o)
                cases += 1
        assert (t["rx"] < 0).any() == (name in ("mag4_full_black", "pyr_whole_black")), name
    for iw, ih, ow, oh in P.SYNTH_REMAPS + [(8, 8, 8, 8)]:
        rx, ry = P.remap_tables(iw, ih, ow, oh, 5)
        ginv, vinv = P.ginv_table(), P.vinv_table(iw * ih)
        for f in P.u8_frames(iw * ih, 13 if iw == 8 else 5, 9):
            for g, v, o in ((1, 1, 1), (0, 0, 0)):
                want = oracle.get_image(f, iw, ih, ow, oh, ginv, vinv, True, True, rx, ry, 1, g, v, o)
                un = P.unmap(f, ginv, vinv, g, v, o)
                assert bits_equal(P.bilinear(un, rx, ry, iw), want) and bits_equal(oracle.undistort(un, rx, ry, iw), want)
                cases += 1
            # the float frames mdc_undistort_batch_device_f32 is given: overexposed pixels kept (section 6) or NaN (section 5)
            fin = oracle.unmap(f, ginv, vinv, True, True, 1, 1, 0 if iw == 8 else 1)
            assert bits_equal(P.bilinear(fin, rx, ry, iw), oracle.undistort(fin, rx, ry, iw)), (iw, ih, ow, oh)
            cases += 1
    print("section 5 (dispatch) and 6: %d frame x flag cases" % cases)
    assert cases == 4 * 5 * 2 + (5 + 5 + 13) * 3
