"""Build recipe for the native libraries (in-tree, no install step).

  libmdc_hip.so    hipcc, gfx950 only   HIP kernels + the C ABI (include/mdc_hip.h); its sources are its build identity (code_id)
  libmdc_host.so   g++                  drop-in C++ classes + C facade (include/mdc_host.h)
  libmdc_multi.so, libmdc_bench.so      one process on N GPUs; measurement and test utilities
  the codec libraries, hipcc, gfx950    libmdc_jenc.so, libmdc_jopt.so, libmdc_zipw.so, libmdc_pngw.so, libmdc_pngw_rgb.so,
                                        libmdc_pnglz.so, libmdc_pngd.so, libmdc_pngdx.so: one translation unit each over shared core
                                        headers, all by one rule (_build_codec), outside libmdc_hip.so's build identity
  libmdc_lens.so, hipcc, gfx950         the RadTan / EquiDistant / pinhole lens models (include/mdc_lens.h), by the same rule
  libmdc_lensinv.so, hipcc, gfx950      the same models and FOV run backwards, raw -> rectified (include/mdc_lensinv.h), by the same rule;
                                        the two share their kernels and host side (csrc/lens_points_shell.h) and differ in the arithmetic
  bin/                                  the programs; tests/native/ programs are built into a place the tests name

All land next to this file so they travel with the source tree to the GPU box.
`python -m mono_dataset_code_amd.build` rebuilds whatever is out of date.
"""
import os
import shutil
import subprocess
import time
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
HOST = os.path.join(CSRC, "host")
INC = os.path.join(ROOT, "include")
EIGEN_STUB = os.path.join(INC, "mono_dataset_code", "compat")  # only used when real Eigen is absent

LIB_HIP = os.path.join(PKG, "libmdc_hip.so")
LIB_HOST = os.path.join(PKG, "libmdc_host.so")

HIP_SOURCES = [os.path.join(CSRC, f) for f in ("mdc_kernels.hip", "mdc_vcal.hip", "mdc_jpeg.hip", "mdc_capi.hip", "mdc_plan.hip", "mdc_launch.hip",
                                                "mdc_pyramid.hip", "mdc_host_calls.hip", "mdc_pipeline.hip", "mdc_placement.hip", "mdc_rcal.hip")]
HIP_DEPS = HIP_SOURCES + [os.path.join(CSRC, "mdc_exports.map"), os.path.join(CSRC, "mdc_internal.h"), os.path.join(CSRC, "mdc_ctx.h"), os.path.join(CSRC, "mdc_build_config.h"), os.path.join(CSRC, "fov_point_model.h"), os.path.join(CSRC, "minmax_first.h"), os.path.join(CSRC, "placement_classes.h"), os.path.join(CSRC, "xcd_placement.h"), os.path.join(INC, "mdc_hip.h")]
HOST_SOURCES = [os.path.join(HOST, f) for f in (
    "fov_undistorter.cpp", "photometric_undistorter.cpp", "gray_png.cpp", "host_device.cpp", "mdc_host_capi.cpp",
    "image_codecs.cpp", "image_codecs_png.cpp", "image_codecs_jpeg.cpp", "image_codecs_jpeg_stream.cpp", "zip_reader.cpp", "image_pool.cpp", "frame_source.cpp", "decode_pool.cpp",
    "prefetch_cache.cpp", "device_lanes.cpp", "batch_run.cpp", "dataset_reader.cpp")]
HOST_DEPS = HOST_SOURCES + [os.path.join(HOST, "mdc_host_exports.map"), os.path.join(HOST, "gray_png.h"), os.path.join(HOST, "host_device.h"),
                            os.path.join(HOST, "image_codecs.h"), os.path.join(HOST, "image_codecs_internal.h"), os.path.join(HOST, "image_codecs_jpeg.h"), os.path.join(HOST, "zip_reader.h"),
                            os.path.join(HOST, "frame_source.h"), os.path.join(HOST, "decode_pool.h"), os.path.join(HOST, "prefetch_cache.h"),
                            os.path.join(HOST, "device_lanes.h"), os.path.join(HOST, "batch_run.h"), os.path.join(HOST, "sibling_library.h"), os.path.join(CSRC, "png_inflate_core.h"),
                            os.path.join(INC, "mono_dataset_code", "BenchmarkDatasetReader.h"),
                            os.path.join(INC, "mdc_hip.h"), os.path.join(INC, "mdc_host.h"), os.path.join(INC, "mdc_lens.h"),
                            os.path.join(INC, "mdc_lensinv.h"), os.path.join(CSRC, "lens_inverse_model.h"),
                            os.path.join(CSRC, "lens_point_model.h"), os.path.join(CSRC, "fov_point_model.h"),
                            os.path.join(INC, "mono_dataset_code", "FOVUndistorter.h"),
                            os.path.join(INC, "mono_dataset_code", "PhotometricUndistorter.h"),
                            os.path.join(INC, "mono_dataset_code", "ExposureImage.h"),
                            os.path.join(INC, "mono_dataset_code", "MdcBind.h")]

# -ffp-contract=off: the reference is built without FMA; contraction would break bit parity.
# -fvisibility=hidden: only what include/mdc_hip.h marks MDC_API is exported (tests/test_abi.py: exported set == header set).
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
             "-fno-fast-math", "-fvisibility=hidden", "-fvisibility-inlines-hidden", "-Wall", "-Wno-unused-function"]
HOST_FLAGS = ["-O2", "-std=c++11", "-ffp-contract=off", "-fPIC", "-shared", "-fvisibility=hidden", "-fvisibility-inlines-hidden", "-Wall"]
HOST_EXPORT_MAP = os.path.join(HOST, "mdc_host_exports.map")
# what still leaks through -fvisibility=hidden (libstdc++ template instantiations are declared with default visibility): made local
EXPORT_MAP = os.path.join(CSRC, "mdc_exports.map")
RECIPE = os.path.abspath(__file__)  # (the flags and mdc_code_id()'s rule live here: a changed recipe relinks, objects are redone by their own rule)


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout)
        raise RuntimeError("build failed: " + " ".join(cmd))
    return r.stdout


def hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def eigen_include():
    """Real Eigen if installed, else the few-type stand-in shipped for this image."""
    for d in ("/usr/include/eigen3", "/usr/local/include/eigen3"):
        if os.path.exists(os.path.join(d, "Eigen", "Core")):
            return d
    return EIGEN_STUB


def code_text(src):
    """C / C++ source without its comments and blank space at line ends (string and character literals kept as they are):
    what the compiler sees of it, so that an edited comment does not make a measured build a different one."""
    out, i, n = [], 0, len(src)
    while i < n:
        c = src[i]
        if c == "/" and i + 1 < n and src[i + 1] == "/":
            while i < n and src[i] != "\n":
                if src[i] == "\\" and i + 1 < n and src[i + 1] == "\n":  # a continued // comment
                    i += 1
                i += 1
        elif c == "/" and i + 1 < n and src[i + 1] == "*":
            j = src.find("*/", i + 2)
            i = n if j < 0 else j + 2
            out.append(" ")
        elif c in "\"'":
            j = i + 1
            while j < n and src[j] != c:
                j += 2 if src[j] == "\\" else 1
            out.append(src[i:j + 1])
            i = j + 1
        elif c in " \t\r\f\v":  # a run of blanks outside literals is one blank
            if not out or out[-1] != " ":
                out.append(" ")
            i += 1
        else:
            out.append(c)
            i += 1
    lines = [l.strip() for l in "".join(out).split("\n")]
    return "\n".join(l for l in lines if l)


def code_id(defines=()):
    """16 hex digits over everything the kernels are made of: sources and shared headers (comments and spacing aside), compile
    flags, -D list, compiler version."""
    import hashlib

    h = hashlib.sha256()
    for path in sorted(HIP_DEPS):
        h.update(os.path.basename(path).encode() + b"\0")
        with open(path, "r", encoding="utf-8", errors="surrogateescape") as f:
            h.update(code_text(f.read()).encode("utf-8", "surrogateescape"))
    h.update(" ".join(HIP_FLAGS + sorted(defines)).encode())
    try:
        h.update(subprocess.run([hipcc(), "--version"], stdout=subprocess.PIPE).stdout)
    except OSError:
        pass
    return h.hexdigest()[:16]


def _linked_from(lib, defines=()):
    """Does `lib` carry the identity of the sources as they are NOW?  (Modification times alone are fooled by an edit that lands while a
    build is running: the objects are from before it, the library's time stamp from after.)"""
    try:
        with open(lib, "rb") as f:
            return code_id(defines).encode() in f.read()
    except OSError:
        return False


def _compile_link_hip(out, defines=(), objdir_tag="product"):
    """Every .hip translation unit -> its own object, in parallel (the kernels TU alone takes a minute), then one link.
    An object is redone when its source, a shared header or the -D list changed."""
    from concurrent.futures import ThreadPoolExecutor

    started = time.time()
    identity = code_id(defines)  # of the sources as the compilers are about to read them
    objdir = os.path.join(PKG, "build", objdir_tag)
    os.makedirs(objdir, exist_ok=True)
    flags = [f for f in HIP_FLAGS if f != "-shared"] + ["-I" + INC] + ["-D" + d for d in defines]
    stamp = os.path.join(objdir, "flags.txt")
    flags_changed = not os.path.exists(stamp) or open(stamp).read() != " ".join(flags)
    headers = [d for d in HIP_DEPS if d not in HIP_SOURCES]
    jobs = []
    for src in HIP_SOURCES:
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        if flags_changed or _stale(obj, [src] + headers) or not os.path.exists(out) or not _linked_from(out, defines):
            jobs.append([hipcc()] + flags + ["-c", src, "-o", obj])
    with ThreadPoolExecutor(max_workers=max(1, len(jobs))) as ex:
        list(ex.map(_run, jobs))
    with open(stamp, "w") as f:
        f.write(" ".join(flags))
    objs = [os.path.join(objdir, os.path.basename(src) + ".o") for src in HIP_SOURCES]
    # mdc_code_id(): the identity of this build (include/mdc_hip.h), a generated one-line translation unit
    idsrc = os.path.join(objdir, "mdc_code_id.cpp")
    with open(idsrc, "w") as f:
        f.write('#include "mdc_hip.h"\nextern "C" const char* mdc_code_id(void) { return "%s"; }\n' % identity)
    idobj = idsrc + ".o"
    _run(["g++", "-O1", "-fPIC", "-fvisibility=hidden", "-I" + INC, "-c", idsrc, "-o", idobj])
    _run([hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + EXPORT_MAP] + objs + [idobj, "-o", out])
    if any(os.path.getmtime(d) > started for d in HIP_DEPS):
        sys.stderr.write("mono_dataset_code_amd.build: a source changed while %s was being built; it is stamped %s and the next build redoes it\n"
                         % (os.path.basename(out), identity))


def build_hip(force=False):
    if force or _stale(LIB_HIP, HIP_DEPS + [RECIPE]) or not _linked_from(LIB_HIP):
        if force:
            shutil.rmtree(os.path.join(PKG, "build", "product"), ignore_errors=True)
        _compile_link_hip(LIB_HIP)
    return LIB_HIP


def build_host(force=False):
    build_hip(force)
    if force or _stale(LIB_HOST, HOST_DEPS + [LIB_HIP]):
        _run(["g++"] + HOST_FLAGS + ["-I" + INC, "-I" + os.path.join(INC, "mono_dataset_code"), "-I" + HOST,
                                     "-I" + eigen_include()] + HOST_SOURCES +
             ["-L" + PKG, "-lmdc_hip", "-Wl,-rpath,$ORIGIN", "-Wl,--version-script=" + HOST_EXPORT_MAP, "-lz", "-lpthread", "-ldl", "-o", LIB_HOST])
    return LIB_HOST


BIN = os.path.join(PKG, "bin")
RESPONSE_CALIB = os.path.join(BIN, "responseCalib")
RESPONSE_CALIB_SOURCE = os.path.join(CSRC, "programs", "responseCalib.cpp")
PLAY_DATASET = os.path.join(BIN, "playDataset")
PLAY_DATASET_SOURCE = os.path.join(CSRC, "programs", "playDataset.cpp")
RECTIFY_DATASET = os.path.join(BIN, "rectifyDataset")
RECTIFY_DATASET_SOURCE = os.path.join(CSRC, "programs", "rectifyDataset.cpp")


def build_programs(force=False):
    """bin/responseCalib: the reference's responseCalib program on top of libmdc_host.so / libmdc_hip.so, and libmdc_pngw.so /
    libmdc_pngw_rgb.so for its result images;
    bin/playDataset: its playDataset program in the saving mode, on top of those and libmdc_jenc.so;
    bin/rectifyDataset: a sequence rectified into a dataset folder (images.zip, camera.txt, ...), on top of those, libmdc_zipw.so,
    libmdc_pngw.so, libmdc_pnglz.so and libmdc_jopt.so."""
    build_host(force)
    build_jenc(force)
    build_jopt(force)
    build_zipw(force)
    build_pngw(force)
    build_pngw_rgb(force)
    build_pnglz(force)
    os.makedirs(BIN, exist_ok=True)
    deps = [RESPONSE_CALIB_SOURCE, LIB_HOST, LIB_HIP, LIB_PNGW, LIB_PNGW_RGB, LIB_ZIPW, os.path.join(INC, "mdc_hip.h"), os.path.join(INC, "mdc_pngw.h"),
            os.path.join(INC, "mdc_pngw_rgb.h"),
            os.path.join(INC, "mono_dataset_code", "BenchmarkDatasetReader.h")]
    if force or _stale(RESPONSE_CALIB, deps):
        _run(["g++", "-O2", "-std=c++11", "-Wall", "-I" + INC, "-I" + os.path.join(INC, "mono_dataset_code"), "-I" + eigen_include(),
              RESPONSE_CALIB_SOURCE, "-L" + PKG, "-lmdc_host", "-lmdc_hip", "-lmdc_zipw", "-lmdc_pngw", "-lmdc_pngw_rgb", "-Wl,-rpath,$ORIGIN/..", "-o",
              RESPONSE_CALIB])
    deps = [PLAY_DATASET_SOURCE, LIB_HOST, LIB_HIP, LIB_JENC, os.path.join(INC, "mdc_hip.h"), os.path.join(INC, "mdc_jenc.h"),
            os.path.join(INC, "mono_dataset_code", "BenchmarkDatasetReader.h")]
    if force or _stale(PLAY_DATASET, deps):
        _run(["g++", "-O2", "-std=c++11", "-Wall", "-I" + INC, "-I" + os.path.join(INC, "mono_dataset_code"), "-I" + eigen_include(),
              PLAY_DATASET_SOURCE, "-L" + PKG, "-lmdc_host", "-lmdc_hip", "-lmdc_jenc", "-Wl,-rpath,$ORIGIN/..", "-o", PLAY_DATASET])
    deps = [RECTIFY_DATASET_SOURCE, LIB_HOST, LIB_HIP, LIB_JENC, LIB_JOPT, LIB_ZIPW, LIB_PNGW, LIB_PNGLZ, os.path.join(INC, "mdc_hip.h"), os.path.join(INC, "mdc_jenc.h"),
            os.path.join(INC, "mdc_jopt.h"),
            os.path.join(INC, "mdc_zipw.h"), os.path.join(INC, "mdc_pngw.h"), os.path.join(INC, "mdc_pnglz.h"), os.path.join(INC, "mono_dataset_code", "BenchmarkDatasetReader.h")]
    if force or _stale(RECTIFY_DATASET, deps):
        _run(["g++", "-O2", "-std=c++11", "-Wall", "-I" + INC, "-I" + os.path.join(INC, "mono_dataset_code"), "-I" + eigen_include(),
              RECTIFY_DATASET_SOURCE, "-L" + PKG, "-lmdc_host", "-lmdc_hip", "-lmdc_jenc", "-lmdc_jopt", "-lmdc_zipw", "-lmdc_pngw", "-lmdc_pnglz", "-Wl,-rpath,$ORIGIN/..", "-o", RECTIFY_DATASET])
    return RESPONSE_CALIB


LIB_BENCH = os.path.join(PKG, "libmdc_bench.so")
BENCH_SOURCE = os.path.join(CSRC, "bench", "mdc_bench.hip")


def build_bench(force=False):
    """libmdc_bench.so: measurement / test utilities (include/mdc_bench.h) -- not part of the product, not linked by it."""
    if force or _stale(LIB_BENCH, [BENCH_SOURCE, os.path.join(INC, "mdc_bench.h"), EXPORT_MAP]):
        _run([hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall", "-I" + INC, BENCH_SOURCE,
              "-Wl,--version-script=" + EXPORT_MAP, "-o", LIB_BENCH])
    return LIB_BENCH


CODEC_HOST = os.path.join(CSRC, "codec_host.h")  # what every codec library's host side has: the last error, the device guard, device resolution


def _build_codec(out, source, deps, export_map, zipw=False, defines=(), force=False, extra_flags=()):
    """One codec library: a single translation unit (`source` and the headers in `deps`), a library of its own outside
    libmdc_hip.so's build identity.  zipw: it stands on libmdc_zipw.so, which is built first and linked.  extra_flags: compiler
    flags beyond the common ones (libmdc_lens.so's floating-point rules)."""
    if zipw:
        build_zipw(force)
    if force or _stale(out, [source, CODEC_HOST] + deps + [export_map] + ([LIB_ZIPW] if zipw else [])):
        _run([hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-fvisibility-inlines-hidden", "-Wall"] +
             list(extra_flags) + ["-D" + d for d in defines] + ["-I" + INC, source] + (["-L" + PKG, "-lmdc_zipw", "-Wl,-rpath,$ORIGIN"] if zipw else []) +
             ["-Wl,--version-script=" + export_map, "-o", out])
    return out


def _build_native_program(source, out, sanitize=True, flags=()):
    """A stand-alone test program of tests/native/ (its own main, pure host code over a header of csrc/), under AddressSanitizer and
    UndefinedBehaviorSanitizer."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    _run(["g++", "-O1", "-g", "-std=c++11", "-Wall", "-Werror"] + list(flags) + san + ["-I" + CSRC, os.path.join(ROOT, "tests", "native", source), "-o", out])
    return out


LIB_JENC = os.path.join(PKG, "libmdc_jenc.so")
JENC_SOURCE = os.path.join(CSRC, "mdc_jenc.hip")
JENC_EXPORT_MAP = os.path.join(CSRC, "mdc_jenc_exports.map")
JPEG_ENCODE_CORE = os.path.join(CSRC, "jpeg_encode_core.h")  # what the two JPEG encoder libraries share: tables, DCT, block walker, scan, host side


def build_jenc(force=False):
    """libmdc_jenc.so: the device baseline JPEG encoder (include/mdc_jenc.h) -- one translation unit, independent of libmdc_hip.so
    and outside its build identity."""
    return _build_codec(LIB_JENC, JENC_SOURCE, [JPEG_ENCODE_CORE, os.path.join(INC, "mdc_jenc.h")], JENC_EXPORT_MAP, force=force)


LIB_JOPT = os.path.join(PKG, "libmdc_jopt.so")
JOPT_SOURCE = os.path.join(CSRC, "mdc_jopt.hip")
JOPT_EXPORT_MAP = os.path.join(CSRC, "mdc_jopt_exports.map")
JOPT_TABLE = os.path.join(CSRC, "jpeg_optimal_table.h")  # the table rule, plain C++: libmdc_jopt.so and a CPU test program


def build_jopt(force=False):
    """libmdc_jopt.so: the device JPEG encoder with per-frame optimal Huffman tables (include/mdc_jopt.h) -- one translation unit,
    the header it shares with mdc_jenc.hip and the table rule's header; it links neither libmdc_jenc.so nor libmdc_hip.so and is
    outside the product's build identity."""
    return _build_codec(LIB_JOPT, JOPT_SOURCE, [JPEG_ENCODE_CORE, JOPT_TABLE, os.path.join(INC, "mdc_jopt.h")], JOPT_EXPORT_MAP, force=force)


def build_jopt_table_program(out, sanitize=True):
    """tests/native/jopt_table.cpp: csrc/jpeg_optimal_table.h (the table rule of libmdc_jopt.so) as a stand-alone program, under
    AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_jopt_cpu.py).  Pure host code."""
    return _build_native_program("jopt_table.cpp", out, sanitize)


LIB_ZIPW = os.path.join(PKG, "libmdc_zipw.so")
ZIPW_SOURCE = os.path.join(CSRC, "mdc_zipw.hip")
ZIPW_EXPORT_MAP = os.path.join(CSRC, "mdc_zipw_exports.map")


def build_zipw(force=False):
    """libmdc_zipw.so: ZIP archives of device-resident files, checksummed and laid out on the device (include/mdc_zipw.h) -- one
    translation unit, independent of every other library here and outside libmdc_hip.so's build identity."""
    return _build_codec(LIB_ZIPW, ZIPW_SOURCE, [os.path.join(INC, "mdc_zipw.h")], ZIPW_EXPORT_MAP, force=force)


LIB_PNGW = os.path.join(PKG, "libmdc_pngw.so")
PNGW_SOURCE = os.path.join(CSRC, "mdc_pngw.hip")
PNGW_EXPORT_MAP = os.path.join(CSRC, "mdc_pngw_exports.map")
PNG_BLOCK = os.path.join(CSRC, "png_block.h")  # the DEFLATE block builder, plain C++: the three PNG encoder libraries and a CPU test program
PNG_ENCODE_CORE = os.path.join(CSRC, "png_encode_core.h")  # what else the three share: filter helpers, stream placement, framing, host helpers


def build_pngw(force=False):
    """libmdc_pngw.so: the device PNG encoder (include/mdc_pngw.h) -- one translation unit and the two headers it shares with
    mdc_pnglz.hip, on top of libmdc_zipw.so (for the IDAT chunk's CRC-32), independent of libmdc_hip.so and outside its build identity."""
    return _build_codec(LIB_PNGW, PNGW_SOURCE, [PNG_BLOCK, PNG_ENCODE_CORE, os.path.join(INC, "mdc_pngw.h"), os.path.join(INC, "mdc_zipw.h")], PNGW_EXPORT_MAP,
                        zipw=True, force=force)


LIB_PNGW_RGB = os.path.join(PKG, "libmdc_pngw_rgb.so")
PNGW_RGB_EXPORT_MAP = os.path.join(CSRC, "mdc_pngw_rgb_exports.map")


def build_pngw_rgb(force=False):
    """libmdc_pngw_rgb.so: the device PNG encoder for 8-bit RGB images (include/mdc_pngw_rgb.h) -- mdc_pngw.hip built with
    -DMDCP_RGB8_LIBRARY, a library of its own beside libmdc_pngw.so (which stays what it is), on top of libmdc_zipw.so."""
    return _build_codec(LIB_PNGW_RGB, PNGW_SOURCE, [PNG_BLOCK, PNG_ENCODE_CORE, os.path.join(INC, "mdc_pngw.h"), os.path.join(INC, "mdc_pngw_rgb.h"),
                                                    os.path.join(INC, "mdc_zipw.h")], PNGW_RGB_EXPORT_MAP, zipw=True, defines=["MDCP_RGB8_LIBRARY=1"], force=force)


LIB_PNGLZ = os.path.join(PKG, "libmdc_pnglz.so")
PNGLZ_SOURCE = os.path.join(CSRC, "mdc_pnglz.hip")
PNGLZ_BLOCK = PNG_BLOCK  # the name the block builder had while it was libmdc_pnglz.so's alone
PNGLZ_EXPORT_MAP = os.path.join(CSRC, "mdc_pnglz_exports.map")


def build_pnglz(force=False):
    """libmdc_pnglz.so: the device PNG encoder with LZ77 matches (include/mdc_pnglz.h), gray and RGB in one library -- one
    translation unit and the two headers it shares with mdc_pngw.hip, on top of libmdc_zipw.so; it links neither libmdc_pngw.so nor
    libmdc_pngw_rgb.so, and it is outside libmdc_hip.so's build identity."""
    return _build_codec(LIB_PNGLZ, PNGLZ_SOURCE, [PNG_BLOCK, PNG_ENCODE_CORE, os.path.join(INC, "mdc_pnglz.h"), os.path.join(INC, "mdc_zipw.h")], PNGLZ_EXPORT_MAP,
                        zipw=True, force=force)


def build_pnglz_block_program(out, sanitize=True):
    """tests/native/pnglz_block.cpp: csrc/png_block.h (the code builder and header writer of the PNG encoder libraries) as a
    stand-alone program, under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_pnglz_cpu.py).  Pure host code."""
    return _build_native_program("pnglz_block.cpp", out, sanitize)


LIB_PNGD = os.path.join(PKG, "libmdc_pngd.so")
PNGD_SOURCE = os.path.join(CSRC, "mdc_pngd.hip")
PNGD_CORE = os.path.join(CSRC, "png_inflate_core.h")
PNGD_EXPORT_MAP = os.path.join(CSRC, "mdc_pngd_exports.map")
PNG_DECODE_KERNELS = os.path.join(CSRC, "png_decode_kernels.h")  # what the two PNG decoder libraries share: the four kernels, the host side


def build_pngd(force=False):
    """libmdc_pngd.so: the device PNG decoder (include/mdc_pngd.h) -- one translation unit, the core header it shares with the CPU
    test program and the kernels' header it shares with mdc_pngdx.hip, independent of every other library here and outside
    libmdc_hip.so's build identity.  The dataset reader loads it at run time (csrc/host/device_lanes.cpp), nothing links it."""
    return _build_codec(LIB_PNGD, PNGD_SOURCE, [PNGD_CORE, PNG_DECODE_KERNELS, os.path.join(INC, "mdc_pngd.h")], PNGD_EXPORT_MAP, force=force)


def build_pngd_core_program(out, sanitize=True):
    """tests/native/pngd_core.cpp: png_inflate_core.h as a stand-alone program (its own main), under AddressSanitizer and
    UndefinedBehaviorSanitizer (tests/test_pngd_cpu.py).  Pure host code: no HIP, no library of ours."""
    return _build_native_program("pngd_core.cpp", out, sanitize)


LIB_PNGDX = os.path.join(PKG, "libmdc_pngdx.so")
PNGDX_SOURCE = os.path.join(CSRC, "mdc_pngdx.hip")
PNGDX_CORE = os.path.join(CSRC, "png_tokens_core.h")  # the token path, phase by phase: libmdc_pngdx.so and a CPU test program
PNGDX_EXPORT_MAP = os.path.join(CSRC, "mdc_pngdx_exports.map")


def build_pngdx(force=False):
    """libmdc_pngdx.so: the device PNG decoder with a parallel inflate for streams with matches (include/mdc_pngdx.h) -- one
    translation unit, the kernels' header it shares with mdc_pngd.hip and the two core headers it shares with the CPU test programs;
    it links neither libmdc_pngd.so nor libmdc_hip.so and is outside the product's build identity.  The dataset reader loads it at
    run time when MDC_GPU_PNG=3 asks for it."""
    return _build_codec(LIB_PNGDX, PNGDX_SOURCE, [PNGD_CORE, PNGDX_CORE, PNG_DECODE_KERNELS, os.path.join(INC, "mdc_pngdx.h")], PNGDX_EXPORT_MAP, force=force)


def build_pngdx_core_program(out, sanitize=True):
    """tests/native/pngdx_core.cpp: png_tokens_core.h (the token path of libmdc_pngdx.so) as a stand-alone program (its own main),
    under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_pngdx_cpu.py).  Pure host code: no HIP, no library of ours."""
    return _build_native_program("pngdx_core.cpp", out, sanitize)


LIB_LENS = os.path.join(PKG, "libmdc_lens.so")
LENS_SOURCE = os.path.join(CSRC, "mdc_lens.hip")
LENS_MODEL = os.path.join(CSRC, "lens_point_model.h")  # the lens arithmetic and the crop rule: libmdc_lens.so, libmdc_host.so and a CPU test program
FOV_MODEL = os.path.join(CSRC, "fov_point_model.h")  # atanf_host_libm (read here, never edited: it is part of libmdc_hip.so's identity)
LENS_SHELL = os.path.join(CSRC, "lens_points_shell.h")  # what the two lens libraries share: the kernels, the launches, the calls' host side
LENS_EXPORT_MAP = os.path.join(CSRC, "mdc_lens_exports.map")
LENS_FP_FLAGS = ["-ffp-contract=off", "-fno-fast-math"]  # IEEE single precision, no FMA: the device gives the host's bits


def build_lens(force=False):
    """libmdc_lens.so: the pinhole / RadTan / EquiDistant lens models on the device (include/mdc_lens.h) -- one translation unit over
    the header it shares with libmdc_host.so and the CPU test program and the shell it shares with mdc_lensinv.hip; it links nothing
    of this project, and it is outside libmdc_hip.so's build identity.  libmdc_host.so loads it at run time for bulk distortCoordinates() calls, nothing links it."""
    return _build_codec(LIB_LENS, LENS_SOURCE, [LENS_SHELL, LENS_MODEL, FOV_MODEL, os.path.join(INC, "mdc_lens.h")], LENS_EXPORT_MAP, force=force, extra_flags=LENS_FP_FLAGS)


def build_lens_core_program(out, sanitize=True):
    """tests/native/lens_core.cpp: lens_point_model.h (the lens arithmetic, the crop rule, the border rules) as a stand-alone program
    (its own main), under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_lens_cpu.py).  Pure host code."""
    return _build_native_program("lens_core.cpp", out, sanitize, flags=LENS_FP_FLAGS)


LIB_LENSINV = os.path.join(PKG, "libmdc_lensinv.so")
LENSINV_SOURCE = os.path.join(CSRC, "mdc_lensinv.hip")
LENSINV_MODEL = os.path.join(CSRC, "lens_inverse_model.h")  # the inverse arithmetic: libmdc_lensinv.so, libmdc_host.so and a CPU test program
LENSINV_EXPORT_MAP = os.path.join(CSRC, "mdc_lensinv_exports.map")


def build_lensinv(force=False):
    """libmdc_lensinv.so: raw pixel -> rectified pixel through the pinhole / RadTan / EquiDistant / FOV lens models on the device
    (include/mdc_lensinv.h) -- one translation unit over the header it shares with libmdc_host.so and the CPU test program and the
    shell it shares with mdc_lens.hip; it links nothing of this project, and it is outside libmdc_hip.so's build identity.  libmdc_host.so loads it at run time for bulk
    undistortCoordinates() calls, nothing links it."""
    return _build_codec(LIB_LENSINV, LENSINV_SOURCE, [LENS_SHELL, LENSINV_MODEL, LENS_MODEL, FOV_MODEL, os.path.join(INC, "mdc_lensinv.h")], LENSINV_EXPORT_MAP, force=force,
                        extra_flags=LENS_FP_FLAGS)


def build_lens_inverse_core_program(out, sanitize=True):
    """tests/native/lens_inverse_core.cpp: lens_inverse_model.h (the inverse arithmetic and the inverse tables' border rules) as a
    stand-alone program (its own main), under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_lens_inverse_cpu.py).
    Pure host code."""
    return _build_native_program("lens_inverse_core.cpp", out, sanitize, flags=LENS_FP_FLAGS)


LIB_MULTI = os.path.join(PKG, "libmdc_multi.so")
MULTI_SOURCE = os.path.join(CSRC, "mdc_multi.hip")


def build_multi(force=False):
    """libmdc_multi.so: one process, N GPUs, RCCL table broadcast (include/mdc_multi.h)."""
    build_hip(force)
    if force or _stale(LIB_MULTI, [MULTI_SOURCE, os.path.join(INC, "mdc_multi.h"), os.path.join(INC, "mdc_hip.h"), LIB_HIP, EXPORT_MAP]):
        rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc())))
        _run([hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall", "-I" + INC, MULTI_SOURCE,
              "-Wl,--version-script=" + EXPORT_MAP,
              "-L" + PKG, "-lmdc_hip", "-L" + os.path.join(rocm, "lib"), "-lrccl", "-lpthread",
              "-Wl,-rpath,$ORIGIN", "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", LIB_MULTI])
    return LIB_MULTI


def build_host_sanitize(out):
    """tests/native/host_sanitize.cpp + the host sources under AddressSanitizer and UndefinedBehaviorSanitizer
    (tests/test_sanitize.py).  The HIP side is the normal libmdc_hip.so, not instrumented."""
    build_hip()
    src = [os.path.join(ROOT, "tests", "native", "host_sanitize.cpp")] + HOST_SOURCES
    _run(["g++", "-O1", "-g", "-std=c++11", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
          "-fno-omit-frame-pointer", "-Wall", "-I" + INC, "-I" + os.path.join(INC, "mono_dataset_code"), "-I" + HOST,
          "-I" + eigen_include()] + src + ["-L" + PKG, "-lmdc_hip", "-Wl,-rpath," + PKG, "-lz", "-lpthread", "-ldl", "-o", out])
    return out


def build_host_tsan(out):
    """tests/native/host_tsan.cpp + the host sources under ThreadSanitizer (tests/test_sanitize.py): the reader's decode pool,
    several readers, the image pool and the decoders from many threads.  The HIP side is the normal libmdc_hip.so."""
    build_hip()
    src = [os.path.join(ROOT, "tests", "native", "host_tsan.cpp")] + HOST_SOURCES
    _run(["g++", "-O1", "-g", "-std=c++11", "-ffp-contract=off", "-fsanitize=thread", "-fno-omit-frame-pointer", "-Wall", "-I" + INC,
          "-I" + os.path.join(INC, "mono_dataset_code"), "-I" + HOST, "-I" + eigen_include()] + src +
         ["-L" + PKG, "-lmdc_hip", "-Wl,-rpath," + PKG, "-lz", "-lpthread", "-ldl", "-o", out])
    return out


def build_variant(name, defines):
    """Experimental build of libmdc_hip with -D switches (see MDC_EXP_* in mdc_kernels.hip);
    loaded by tools/sweep.py --lib.  Lands in mono_dataset_code_amd/variants/."""
    d = os.path.join(PKG, "variants")
    os.makedirs(d, exist_ok=True)
    out = os.path.join(d, "libmdc_hip_%s.so" % name)
    diag = [] if name == "debug" else ["MDC_DIAGNOSIS_BUILD=1"]
    if _stale(out, HIP_DEPS + [RECIPE]) or not _linked_from(out, diag + list(defines)):
        # MDC_DIAGNOSIS_BUILD: the licence for the wrong-result switches of csrc/mdc_build_config.h -- only ever set here,
        # for a library that lands under variants/ and reports itself through mdc_build_flags()
        _compile_link_hip(out, diag + list(defines), objdir_tag="variant_" + name)
    return out


def build_debug():
    """The bounds-checking build of the kernels (tests/test_gpu_debug.py); travels to the GPU box like the product build."""
    return build_variant("debug", ["MDC_DEBUG_BOUNDS=1"])


def build_fault_injection():
    """libmdc_hip with MDC_EXP_HUFF_BAD_PROVISIONAL: the split Huffman kernel's segments publish wrong provisional exit states, so every
    right neighbour takes the path that relaxes a third time from the final state (tests/test_reader.py); right results, slower."""
    return build_variant("badprov", ["MDC_EXP_HUFF_BAD_PROVISIONAL=1"])


def build_huff_rounds():
    """libmdc_hip with MDC_EXP_HUFF_ROUNDS: the one-workgroup-per-frame Huffman kernel reports its relaxation rounds in the status
    word's upper bits (tests/test_jdec.py); right records."""
    return build_variant("huffrounds", ["MDC_EXP_HUFF_ROUNDS=1"])


def build_all(force=False):
    build_hip(force)
    build_host(force)
    build_programs(force)
    build_multi(force)
    build_bench(force)
    build_jenc(force)
    build_jopt(force)
    build_zipw(force)
    build_pngw(force)
    build_pngw_rgb(force)
    build_pnglz(force)
    build_pngd(force)
    build_pngdx(force)
    build_lens(force)
    build_lensinv(force)
    build_debug()
    build_fault_injection()
    build_huff_rounds()
    return LIB_HIP, LIB_HOST, LIB_MULTI


if __name__ == "__main__":
    print("\n".join(build_all(force="--force" in sys.argv)))
