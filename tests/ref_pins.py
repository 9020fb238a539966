"""The reference build's answers, recorded, for machines where it cannot be built.

oracle/_ref/libmdc_ref.so is compiled from the reference's own sources, which only the build container has.  The `ref` fixture
(conftest.py) hands the tests a PinnedRef with the same interface as oracle.loader.Ref:

  live     (the reference build is there): every call goes to the reference build, and its answer must equal the answer recorded
           in tests/golden/ref_pins.json for the same call.  MDC_RECORD_REF_PINS=1 records instead, adding this session's answers
           to the file; MDC_RECORD_REF_PINS=fresh writes this session's answers alone (stale ones dropped: use it on a run of the
           whole suite, GPU tests included, where the reference build is present);
  replay   (it is not): small answers (validity, sizes, intrinsics) come from the recording; a large array is computed by this
           repository (its host classes for the tables, the C oracle for the per-frame functions) and must have the recorded
           answer's digest, so it IS the reference's array, bit for bit (NaN payloads aside, as in conftest.bits_equal).

A call is identified by its method, the contents of the files it reads and digests of the arrays it is given.  What the reference
leaves undefined is not pinned: an invalid camera's output size (UndistorterFOV never sets it)."""
import atexit
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = os.path.join(HERE, "golden", "ref_pins.json")
SMALL = 64  # arrays up to this many elements are recorded verbatim


def _h(data, n=16):
    return hashlib.sha256(data).hexdigest()[:n]


def array_digest(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = a.copy()
        a[np.isnan(a)] = np.nan  # one NaN pattern: the payload of a propagated NaN is not specified
    return _h(("%s%s" % (a.dtype.str, a.shape)).encode() + a.tobytes(), 24)


def arg_key(x):
    if isinstance(x, (PinnedFov, PinnedPhoto)):
        return x.key
    if isinstance(x, np.ndarray):
        return "a" + array_digest(x)
    if isinstance(x, str):
        try:
            with open(x, "rb") as f:
                return "f" + _h(f.read())
        except OSError:
            pass
        if os.sep in x:
            return "f-" + os.path.basename(x)  # a missing file: by its name (the directory is a temporary one)
        return "s" + repr(x)
    return repr(x)


def encode(v):
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (np.integer, np.floating)):
        return v.item()
    if isinstance(v, (tuple, list)):
        return [encode(x) for x in v]
    if isinstance(v, dict):
        return {k: encode(x) for k, x in sorted(v.items())}
    a = np.asarray(v)
    if a.size <= SMALL:
        bits = a.view(np.uint32) if a.dtype == np.float32 else a
        return {"dtype": a.dtype.str, "shape": list(a.shape), "bits": bits.ravel().tolist()}
    return {"digest": array_digest(a)}


def decode(e):
    if isinstance(e, list):
        return [decode(x) for x in e]
    if isinstance(e, dict) and "bits" in e:
        dt = np.dtype(e["dtype"])
        raw = np.array(e["bits"], np.uint32 if dt == np.float32 else dt)
        return (raw.view(np.float32) if dt == np.float32 else raw).reshape(e["shape"])
    if isinstance(e, dict) and "digest" in e:
        raise AssertionError("a recorded array digest cannot be replayed without computing the array")
    if isinstance(e, dict):
        return {k: decode(x) for k, x in e.items()}
    return e


RECORD = os.environ.get("MDC_RECORD_REF_PINS", "")
_recorded = {}  # this session's answers (every Pins of the process), written once at exit


def _save():
    table = {}
    if RECORD != "fresh" and os.path.exists(PINS):
        with open(PINS) as f:
            table = json.load(f)
    table.update(_recorded)
    with open(PINS, "w") as f:
        json.dump(dict(sorted(table.items())), f, indent=0, separators=(",", ":"))
        f.write("\n")


if RECORD in ("1", "fresh"):
    atexit.register(_save)


class Pins:
    def __init__(self, live):
        self.live = live
        self.record = live is not None and RECORD in ("1", "fresh")
        with open(PINS) if os.path.exists(PINS) else _empty() as f:
            self.table = json.load(f)

    def answer(self, call, live_fn, ours_fn=None):
        """The reference's answer to `call` (a string naming it): live_fn() checked against the recording, or the recording itself, or
        ours_fn() checked against the recording."""
        key = _h(call.encode())
        if self.live is not None:
            v = live_fn()
            if self.record:
                _recorded[key] = encode(v)
            else:
                assert key in self.table, "no recorded answer of the reference for %s: run the suite once with MDC_RECORD_REF_PINS=1" % call
                assert encode(v) == self.table[key], "the reference build's answer to %s is not the recorded one" % call
            return v
        assert key in self.table, "no recorded answer of the reference for %s (and no reference build here)" % call
        rec = self.table[key]
        if ours_fn is None or rec is None or not _has_digest(rec):
            return _shape_like(decode(rec))
        v = ours_fn()
        assert encode(v) == rec, "this repository's answer to %s differs from the reference's recorded one" % call
        return v


def _has_digest(e):
    if isinstance(e, dict):
        return "digest" in e or any(_has_digest(x) for x in e.values())
    if isinstance(e, list):
        return any(_has_digest(x) for x in e)
    return False


def _shape_like(v):
    return tuple(v) if isinstance(v, list) else v


class _empty:
    def __enter__(self):
        import io

        return io.StringIO("{}")

    def __exit__(self, *a):
        return False


class PinnedRef:
    """oracle.loader.Ref's interface over the reference build (live) or the recording (replay)."""

    def __init__(self, live=None):
        self.live = live
        self.pins = Pins(live)
        self._oracle = None

    @property
    def oracle(self):
        if self._oracle is None:
            from oracle import loader

            self._oracle = loader.Oracle()
        return self._oracle

    def fov(self, camera_txt):
        return PinnedFov(self, camera_txt)

    def photo(self, pcalib, vignette, w, h):
        return PinnedPhoto(self, pcalib, vignette, w, h)

    def get_image(self, fov, photo, raw, rectify, g, v, o, out=None):
        call = "get_image(%s)" % ",".join(arg_key(a) for a in (fov, photo, raw, rectify, g, v, o))

        def ours():
            iw, ih, ow, oh = fov.ours().dims()
            rm = fov.ours().remap()
            rx, ry = rm if rm is not None else (None, None)
            p = photo.ours()
            valid = p.valid()
            vig = p.vignette() if valid & 2 else None
            return self.oracle.get_image(raw, iw, ih, ow, oh, p.ginv() if valid & 1 else None, vig[1] if vig else None, valid & 1, valid & 2,
                                         rx, ry, rectify, g, v, o)

        got = self.pins.answer(call, lambda: self.live.get_image(fov.live, photo.live, raw, rectify, g, v, o), ours)
        if out is not None:
            out[...] = got
            return out
        return got


class PinnedFov:
    def __init__(self, R, camera_txt):
        self.R, self.path = R, camera_txt
        self.key = "fov(%s)" % arg_key(camera_txt)
        self.live = R.live.fov(camera_txt) if R.live is not None else None
        self._ours = None

    def ours(self):
        """this repository's UndistorterFOV on the same file (replay only)"""
        if self._ours is None:
            from mono_dataset_code_amd import capi

            self._ours = capi.UndistorterFOV(self.path)
        return self._ours

    def _answer(self, name, args, live_fn, ours_fn=None):
        return self.R.pins.answer("%s.%s(%s)" % (self.key, name, ",".join(arg_key(a) for a in args)), live_fn, ours_fn)

    def is_valid(self):
        return self._answer("is_valid", (), lambda: self.live.is_valid())

    def dims(self):
        """(in_w, in_h, out_w, out_h); for an invalid camera only the input size is defined (and pinned) -- the reference never sets
        the output size then, so live it is whatever the memory held and in replay it is not there (a 2-tuple)"""
        valid = self.is_valid()
        full = []

        def live():
            full.append(tuple(self.live.dims()))
            return full[0] if valid else full[0][:2]

        got = tuple(self._answer("dims", (), live))
        return full[0] if full else got

    def intrinsics(self):
        return self._answer("intrinsics", (), lambda: self.live.intrinsics())

    def remap(self):
        got = self._answer("remap", (), lambda: self.live.remap(), lambda: self.ours().remap())
        return tuple(got) if got is not None else None

    def distort_coordinates(self, x, y):
        def ours():
            self.ours().distort_coordinates(x, y)
            return x, y

        def live():
            self.live.distort_coordinates(x, y)
            return x, y

        got = self._answer("distort_coordinates", (x, y), live, ours)
        x[...], y[...] = got[0], got[1]

    def undistort(self, img, out):
        def ours():
            W, H, w, h = self.ours().dims()
            if img.size == W * H and out.size == w * h:  # wrong sizes: output untouched (src/FOVUndistorter.cpp:327-338)
                rx, ry = self.ours().remap()
                out[...] = self.R.oracle.undistort(img, rx, ry, W)
            return out

        def live():
            self.live.undistort(img, out)
            return out

        got = self._answer("undistort", (img, out), live, ours)
        out[...] = got


class PinnedPhoto:
    def __init__(self, R, pcalib, vignette, w, h):
        self.R, self.args = R, (pcalib, vignette, w, h)
        self.key = "photo(%s)" % ",".join(arg_key(a) for a in self.args)
        self.live = R.live.photo(pcalib, vignette, w, h) if R.live is not None else None
        self._ours = None

    def ours(self):
        """this repository's PhotometricUndistorter on the same files (replay only)"""
        if self._ours is None:
            from mono_dataset_code_amd import capi

            self._ours = capi.PhotometricUndistorter(*self.args)
        return self._ours

    def _answer(self, name, args, live_fn, ours_fn=None):
        return self.R.pins.answer("%s.%s(%s)" % (self.key, name, ",".join(arg_key(a) for a in args)), live_fn, ours_fn)

    def valid(self):
        return self._answer("valid", (), lambda: self.live.valid())

    def ginv(self):
        return self._answer("ginv", (), lambda: self.live.ginv(), lambda: self.ours().ginv())

    def g(self):
        return self._answer("g", (), lambda: self.live.g(), lambda: self.ours().g())

    def vignette(self):
        got = self._answer("vignette", (), lambda: self.live.vignette(), lambda: self.ours().vignette())
        return tuple(got) if got is not None else None

    def unmap(self, img, out, g, v, o):
        def ours():
            p = self.ours()
            valid = p.valid()
            vig = p.vignette() if valid & 2 else None
            out[...] = self.R.oracle.unmap(img, p.ginv() if valid & 1 else None, vig[1] if vig else None, valid & 1, valid & 2, g, v, o)
            return out

        def live():
            self.live.unmap(img, out, g, v, o)
            return out

        got = self._answer("unmap", (img, out, g, v, o), live, ours)
        out[...] = got


class PinnedVcalRef:
    """oracle.loader.VcalRef's interface (the reference's vignetteCalib loops) over its build or the recording; replay computes with the
    C oracle's restatement of the same loops."""

    def __init__(self, live=None):
        self.live = live
        self.pins = Pins(live)
        self._oracle = None

    @property
    def oracle(self):
        if self._oracle is None:
            from oracle import loader

            self._oracle = loader.Oracle()
        return self._oracle

    def _answer(self, name, args, live_fn, ours_fn):
        return tuple(self.pins.answer("vcal.%s(%s)" % (name, ",".join(arg_key(a) for a in args)), live_fn, ours_fn))

    def plane_step(self, images, p2x, p2y, gw, gh, plane_color, vig, oth2):
        args = (images, p2x, p2y, gw, gh, plane_color, vig, oth2)
        return self._answer("plane_step", args, lambda: self.live.plane_step(*args),
                            lambda: self.oracle.vcal_plane_step(images, p2x, p2y, plane_color, vig, oth2))

    def vignette_step(self, images, p2x, p2y, gw, gh, plane_color, vig, oth2):
        args = (images, p2x, p2y, gw, gh, plane_color, vig, oth2)
        return self._answer("vignette_step", args, lambda: self.live.vignette_step(*args),
                            lambda: self.oracle.vcal_vignette_step(images, p2x, p2y, plane_color, vig, oth2))

    def smooth(self, vig, wI, hI):
        return self._answer("smooth", (vig, wI, hI), lambda: self.live.smooth(vig, wI, hI), lambda: self.oracle.vcal_smooth(vig, wI, hI))

    def mask_coords(self, x, y, gw, gh, wI, hI):
        return self._answer("mask_coords", (x, y, gw, gh, wI, hI), lambda: self.live.mask_coords(x, y, gw, gh, wI, hI),
                            lambda: self.oracle.vcal_mask_coords(x, y, wI, hI))

    def gradient_mask(self, image, max_abs_grad):
        return self.pins.answer("vcal.gradient_mask(%s)" % ",".join(arg_key(a) for a in (image, max_abs_grad)),
                                lambda: self.live.gradient_mask(image, max_abs_grad), lambda: self.oracle.vcal_gradient_mask(image, max_abs_grad))
