#!/usr/bin/env python3
"""Decode-only rate of the reader's prefetch path, no GPU needed: getImageRaw in order over a folder of 1280x1024 PNGs
(mdch_reader_get_raw of include/mdc_host.h), frames/s.  One process per run, so that two builds of libmdc_host.so can be run
alternately.  usage: python tools/raw_decode_rate.py [path of libmdc_host.so] [frames (default 64)] [passes (default 3)]"""
import ctypes
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

from mono_dataset_code_amd import synth  # noqa: E402

LIB = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "mono_dataset_code_amd", "libmdc_host.so")
N = int(sys.argv[2]) if len(sys.argv) > 2 else 64
PASSES = int(sys.argv[3]) if len(sys.argv) > 3 else 3

d = tempfile.mkdtemp(prefix="mdc_raw_")
synth.write_sequence_calibration(d, synth.CAMERA_1280_TO_640, n_times=N)
os.makedirs(os.path.join(d, "images"))
y, x = np.mgrid[0:1024, 0:1280]
for i in range(N):
    rng = np.random.default_rng(i % 8)
    img = np.clip(127 + 100 * np.sin(0.01 * x + i % 8) * np.cos(0.013 * y) + rng.normal(0, 4, (1024, 1280)), 0, 255).astype(np.uint8)
    Image.fromarray(img).save(os.path.join(d, "images", "%05d.png" % i), compress_level=1)

lib = ctypes.CDLL(LIB)
lib.mdch_reader_create.restype = ctypes.c_void_p
lib.mdch_reader_create.argtypes = [ctypes.c_char_p]
lib.mdch_reader_get_raw.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.POINTER(ctypes.c_int)]
lib.mdch_reader_destroy.argtypes = [ctypes.c_void_p]
reader = lib.mdch_reader_create((d + "/").encode())
out = np.empty(1280 * 1024, np.uint8)
wh = (ctypes.c_int * 2)()


def walk():
    good = 0
    for i in range(N):
        good += lib.mdch_reader_get_raw(reader, i, out.ctypes.data, out.size, wh)
    return good


walk()  # warm: page cache, the pool's threads
t0 = time.perf_counter()
good = sum(walk() for _ in range(PASSES))
dt = time.perf_counter() - t0
print("RAW_DECODE_RATE %s: %d of %d frames in %.3f s = %.1f frames/s" % (LIB, good, N * PASSES, dt, N * PASSES / dt))
lib.mdch_reader_destroy(reader)
