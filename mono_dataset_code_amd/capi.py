"""ctypes bindings of include/mdc_hip.h (libmdc_hip.so) and include/mdc_host.h (libmdc_host.so).

Thin, explicit, no logic: every Python method is one C call.  Device buffers are
passed as integer addresses (e.g. torch.Tensor.data_ptr()), host buffers as numpy
arrays.  Loading fails loudly (OSError) when the libraries have not been built --
there is no Python or CPU fallback for the per-frame work.
"""
import ctypes as C
import os
import types

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_HIP_PATH = os.environ.get("MDC_LIB_HIP") or os.path.join(_PKG, "libmdc_hip.so")  # override: experiment builds
LIB_HOST_PATH = os.path.join(_PKG, "libmdc_host.so")

# flag word (include/mdc_hip.h)
GAMMA, VIGNETTE, KILL_OVEREXPOSED, RECTIFY = 1, 2, 4, 8
KERNEL_AUTO, KERNEL_GATHER, KERNEL_TILED = 0, 1, 2
OPT_KERNEL, OPT_FRAMES_PER_BLOCK, OPT_TILE_ROWS, OPT_TILE_ORDER, OPT_WINDOW_BUFFERS, OPT_FRAME_INTERLEAVE, OPT_TILE_COLS, OPT_PIN_CALLER_BUFFERS = 1, 2, 5, 6, 7, 8, 9, 10
OPT_TWO_STAGE = 11
OPT_PREFETCH_CHUNK = 12
OPT_PREFETCH_STREAMS = 13
OPT_ZERO_COPY = 14
OPT_TAIL_TAPER = 15
OPT_XCD_ROTATE = 18
OPT_DEVICE_PIPELINE_CHUNK, OPT_DEVICE_PIPELINE_CHUNK_HINT = 16, 17
ORDER_BANDS, ORDER_ROWS, ORDER_IDENTITY, ORDER_BLOCKS2D = 0, 1, 2, 3
OK, ERR_ARG, ERR_STATE, ERR_SIZE, ERR_HIP, ERR_NO_DEVICE, ERR_NOMEM = 0, -1, -2, -3, -4, -5, -6

PLACE_AUTO, PLACE_FIRST, PLACE_MALLOC, PLACE_VMM = 0, 1, 2, 3
PLACE_NAMES = {PLACE_AUTO: "auto", PLACE_FIRST: "first", PLACE_MALLOC: "malloc", PLACE_VMM: "vmm"}


RCAL_EXACT_ORDER, RCAL_DIRECT = 0, 1


class RcalIter(C.Structure):
    """mdc_rcal_iter (include/mdc_hip.h)"""
    _fields_ = [(n, C.c_double) for n in ("rmse_G", "num_G", "rmse_E", "num_E", "rmse_resc", "num_resc", "rescale")]


class RcalLog(C.Structure):
    """mdc_rcal_log (include/mdc_hip.h)"""
    _fields_ = [("init_rmse", C.c_double), ("init_num", C.c_double), ("iters", C.POINTER(RcalIter))]


class PlacedBuffers(C.Structure):
    """mdc_placed_buffers (include/mdc_hip.h)"""
    _fields_ = [("d_in", C.c_void_p), ("d_out", C.c_void_p), ("in_bytes", C.c_size_t), ("out_bytes", C.c_size_t), ("nframes", C.c_int64),
                ("probe_frames", C.c_int64), ("strategy", C.c_int), ("candidates_in", C.c_int), ("candidates_out", C.c_int), ("picked_in", C.c_int),
                ("picked_out", C.c_int), ("pair_ms", C.c_float * 64), ("pieces", C.c_int), ("piece_mib", C.c_int), ("class_count", C.c_int * 3),
                ("ms_first", C.c_float), ("ms_chosen", C.c_float), ("note", C.c_char * 384), ("handle", C.c_void_p)]

    def describe(self):
        """what was done, for a bench line / a log"""
        d = {"strategy": PLACE_NAMES.get(self.strategy, str(self.strategy)), "how": self.note.decode(errors="replace"),
             "probe_frames": int(self.probe_frames), "ms_on_first_allocations": round(float(self.ms_first), 4) or None,
             "ms_on_chosen_pair": round(float(self.ms_chosen), 4) or None}
        if self.strategy == PLACE_MALLOC and self.candidates_in > 1:
            ki, ko = self.candidates_in, self.candidates_out
            d["ms_frames_i_results_j"] = [[round(float(self.pair_ms[i * ko + j]), 4) for j in range(ko)] for i in range(ki)]
            d["picked_frames"], d["picked_results"] = int(self.picked_in), int(self.picked_out)
        if self.strategy == PLACE_VMM:
            d["pieces"], d["piece_mib"], d["class_count"] = int(self.pieces), int(self.piece_mib), [int(x) for x in self.class_count]
        return d


class StripedSet(C.Structure):
    """mdc_striped_set (include/mdc_hip.h)"""
    _fields_ = [("n", C.c_int), ("d_ptr", C.c_void_p * 16), ("bytes", C.c_size_t * 16), ("strategy", C.c_int), ("pieces", C.c_int), ("piece_mib", C.c_int),
                ("class_count", C.c_int * 3), ("note", C.c_char * 384), ("handle", C.c_void_p)]


class FovModel(C.Structure):
    _fields_ = [("in_calib", C.c_float * 5), ("in_w", C.c_int), ("in_h", C.c_int), ("out_calib", C.c_float * 5),
                ("out_w", C.c_int), ("out_h", C.c_int)]


LENS_PINHOLE, LENS_RADTAN, LENS_EQUIDISTANT = 0, 1, 2  # MDCN_PINHOLE, MDCN_RADTAN, MDCN_EQUIDISTANT
LENS_NAMES = {0: "FOV / pinhole", 1: "RadTan", 2: "EquiDistant"}  # UndistorterFOV.lens_model()
LENSINV_PINHOLE, LENSINV_RADTAN, LENSINV_EQUIDISTANT, LENSINV_FOV = 0, 1, 2, 3  # MDCU_PINHOLE, MDCU_RADTAN, MDCU_EQUIDISTANT, MDCU_FOV


class LensModel(C.Structure):
    """include/mdc_lens.h: mdcn_model -- a raw camera (pinhole, RadTan or EquiDistant) and the rectified pinhole, in pixels.
    include/mdc_lensinv.h: mdcu_model has the same 17 words, and the kind LENSINV_FOV with k[0] = omega beside the three."""
    _fields_ = [("kind", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("k", C.c_float * 4),
                ("in_w", C.c_int), ("in_h", C.c_int), ("ofx", C.c_float), ("ofy", C.c_float), ("ocx", C.c_float), ("ocy", C.c_float),
                ("out_w", C.c_int), ("out_h", C.c_int)]

    @classmethod
    def make(cls, kind, cam, rect, in_size=(0, 0), out_size=(0, 0)):
        """cam = fx fy cx cy k0 k1 k2 k3, rect = ofx ofy ocx ocy"""
        m = cls()
        m.kind = int(kind)
        m.fx, m.fy, m.cx, m.cy = (float(v) for v in cam[:4])
        for i in range(4):
            m.k[i] = float(cam[4 + i])
        m.ofx, m.ofy, m.ocx, m.ocy = (float(v) for v in rect)
        (m.in_w, m.in_h), (m.out_w, m.out_h) = in_size, out_size
        return m


class MdcInfo(C.Structure):
    _fields_ = [("device", C.c_int), ("in_w", C.c_int), ("in_h", C.c_int), ("out_w", C.c_int), ("out_h", C.c_int),
                ("valid_gamma", C.c_int), ("valid_vignette", C.c_int), ("valid_remap", C.c_int), ("tiled", C.c_int),
                ("tile_w", C.c_int), ("tile_h", C.c_int), ("n_tiles", C.c_int), ("lds_bytes", C.c_int),
                ("window_buffers", C.c_int), ("f32_tiled", C.c_int), ("f32_tile_w", C.c_int), ("f32_tile_h", C.c_int),
                ("src_bbox", C.c_int * 4), ("src_bbox_bytes", C.c_int64), ("src_staged_bytes", C.c_int64),
                ("n_black", C.c_int64), ("two_stage", C.c_int), ("prefetch_chunk", C.c_int), ("prefetch_streams", C.c_int)]


class DeviceOutputs(C.Structure):
    """include/mdc_hip.h: mdc_device_outputs -- device arrays the *_to_device calls / DatasetReader.get_images_device fill."""
    _fields_ = [("base", C.c_void_p), ("levels", C.c_int), ("level", C.c_void_p * 3), ("dI", C.c_void_p * 4), ("abs_squared_grad", C.c_void_p * 4)]

    @classmethod
    def make(cls, base, levels=1, level=(), dI=(), abs2=()):
        o = cls()
        o.base, o.levels = base, levels
        for i, p in enumerate(level):
            o.level[i] = p
        for i, p in enumerate(dI):
            o.dI[i] = p
        for i, p in enumerate(abs2):
            o.abs_squared_grad[i] = p
        return o


class TuneResult(C.Structure):
    _fields_ = [("tile_w", C.c_int), ("tile_h", C.c_int), ("frames_per_block", C.c_int), ("ms", C.c_float), ("candidates", C.c_int)]


class MdcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mdc error %d: %s" % (code, msg))
        self.code = code


_vp, _i, _i64, _u32, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_size_t
_u, _f, _cp, _P = C.c_uint, C.c_float, C.c_char_p, C.POINTER

# The signatures, name -> (restype, argtypes): the one place an entry point is declared on the Python side, one row each, in
# the order and under the section comments of its header.  tests/test_abi.py checks every row against the header's declaration.
HIP_API = {  # include/mdc_hip.h (libmdc_hip.so)
    # ---- lifetime
    "mdc_create": (_i, [_i, _P(_vp)]),
    "mdc_device_count": (_i, []),
    "mdc_device_pci_bus_id": (_i, [_vp, _cp, _sz]),
    "mdc_destroy": (None, [_vp]),
    "mdc_last_error": (_cp, [_vp]),
    "mdc_get_info": (_i, [_vp, _P(MdcInfo)]),
    "mdc_set_option": (_i, [_vp, _i, _i]),
    "mdc_build_flags": (_cp, []),
    "mdc_code_id": (_cp, []),
    # ---- calibration tables (once per sequence)
    "mdc_set_photometric": (_i, [_vp, _vp, _vp, _i, _i]),
    "mdc_set_remap": (_i, [_vp, _vp, _vp, _i, _i, _i, _i]),
    # ---- host-pointer, single-frame
    "mdc_unmap_host": (_i, [_vp, _vp, _vp, _i, _u]),
    "mdc_undistort_host_f32": (_i, [_vp, _vp, _vp, _i, _i]),
    "mdc_undistort_host_u8": (_i, [_vp, _vp, _vp, _i, _i]),
    "mdc_process_host": (_i, [_vp, _vp, _vp, _u]),
    # ---- host-pointer, many frames
    "mdc_host_alloc": (_vp, [_sz]),
    "mdc_host_free": (None, [_vp]),
    "mdc_process_frames_host": (_i, [_vp, _P(_vp), _P(_vp), _i64, _u]),
    "mdc_process_jpeg_frames_host": (_i, [_vp, _P(_vp), _i64, _i, _i, _P(_vp), _i64, _u]),
    "mdc_jpeg_idct_batch_device": (_i, [_vp, _vp, _i64, _vp, _i, _i, _i, _i, _i64, _vp]),
    "mdc_process_jpeg_streams_host": (_i, [_vp, _P(_vp), _P(_i64), _P(_vp), _i64, _u, _P(_i)]),
    "mdc_jpeg_huffman_batch_device": (_i, [_vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i64, _vp, _vp]),
    # ---- host frames in, results left on the device
    "mdc_process_frames_host_to_device": (_i, [_vp, _P(_vp), _i64, _u, _P(DeviceOutputs), _P(_i64)]),
    "mdc_process_jpeg_frames_host_to_device": (_i, [_vp, _P(_vp), _i64, _i, _i, _i64, _u, _P(DeviceOutputs), _P(_i64)]),
    "mdc_process_jpeg_streams_host_to_device": (_i, [_vp, _P(_vp), _P(_i64), _i64, _u, _P(DeviceOutputs), _P(_i64), _P(_i)]),
    "mdc_device_alloc": (_i, [_vp, _sz, _P(_vp)]),
    "mdc_tune_placement_device": (_i, [_vp, _P(_vp), _i, _P(_vp), _i, _i64, _u, _vp, _P(_i), _P(_i), _P(_f)]),
    "mdc_alloc_placed_device": (_i, [_vp, _sz, _sz, _i64, _u, _i, _vp, _P(PlacedBuffers)]),
    "mdc_free_placed_device": (_i, [_vp, _P(PlacedBuffers)]),
    "mdc_alloc_striped_set_device": (_i, [_vp, _i, _P(_sz), _vp, _P(StripedSet)]),
    "mdc_free_striped_set_device": (_i, [_vp, _P(StripedSet)]),
    "mdc_device_free": (None, [_vp, _vp]),
    "mdc_copy_to_host": (_i, [_vp, _vp, _vp, _sz]),
    # ---- device-pointer, batched: the throughput path
    "mdc_unmap_batch_device": (_i, [_vp, _vp, _vp, _i64, _u, _vp]),
    "mdc_process_batch_device": (_i, [_vp, _vp, _vp, _i64, _u, _vp]),
    "mdc_undistort_batch_device_f32": (_i, [_vp, _vp, _vp, _i64, _vp]),
    "mdc_pyramid_batch_device": (_i, [_vp, _vp, _i, _i, _i, _P(_vp), _i64, _vp]),
    "mdc_process_pyramid_batch_device": (_i, [_vp, _vp, _vp, _i, _P(_vp), _i64, _u, _vp]),
    "mdc_gradients_batch_device": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i64, _vp]),
    "mdc_process_pyramid_gradients_batch_device": (_i, [_vp, _vp, _vp, _i, _P(_vp), _P(_vp), _P(_vp), _i64, _u, _i, _vp]),
    # ---- lens model on many points
    "mdc_distort_points_device": (_i, [_vp, _P(FovModel), _vp, _vp, _i64, _vp]),
    "mdc_distort_points_host": (_i, [_vp, _P(FovModel), _vp, _vp, _i64]),
    # ---- vignetteCalib solver
    "mdc_vcal_plane_step_device": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "mdc_vcal_vignette_step_device": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "mdc_vcal_index_create": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _P(_vp)]),
    "mdc_vcal_index_destroy": (None, [_vp]),
    "mdc_vcal_index_bytes": (_i64, [_vp]),
    "mdc_vcal_index_entries": (_i64, [_vp]),
    "mdc_vcal_vignette_step_indexed_device": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "mdc_vcal_solve_device": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp, _vp]),
    "mdc_vcal_scale_images_device": (_i, [_vp, _vp, _i, _i64, _f, _vp, _vp]),
    "mdc_vcal_gradient_mask_device": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "mdc_vcal_mask_coords_device": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp]),
    "mdc_vcal_plane_coords_device": (_i, [_vp, _P(FovModel), _vp, _vp, _i, _i, _i, _f, _f, _vp, _vp, _vp]),
    "mdc_vcal_smooth_device": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "mdc_vcal_plot_plane_device": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "mdc_vcal_vignette_u16_device": (_i, [_vp, _vp, _i64, _vp, _vp]),
    # ---- responseCalib solver
    "mdc_rcal_leak_pad_device": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "mdc_rcal_init_e_device": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "mdc_rcal_rmse_device": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "mdc_rcal_g_step_device": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "mdc_rcal_index_create": (_i, [_vp, _vp, _i, _i, _i, _vp, _P(_vp)]),
    "mdc_rcal_index_destroy": (None, [_vp]),
    "mdc_rcal_index_bytes": (_i64, [_vp]),
    "mdc_rcal_index_entries": (_i64, [_vp]),
    "mdc_rcal_index_longest_chain": (_i64, [_vp]),
    "mdc_rcal_g_step_indexed_device": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "mdc_rcal_e_step_device": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "mdc_rcal_rescale_device": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "mdc_rcal_solve_device": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _u, _vp, _vp, _P(RcalLog), _vp]),
    "mdc_rcal_plot_e_device": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "mdc_rcal_plot_g_device": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "mdc_copy_to_device": (_i, [_vp, _vp, _vp, _sz]),
    # ---- plan selection by measurement, diagnostics
    "mdc_tune_device": (_i, [_vp, _vp, _vp, _i64, _u, _vp, _P(TuneResult)]),
    "mdc_describe_launch": (_i, [_vp, _u, _i, _cp, _sz]),
    # ---- calibration hand-over between ranks (multi-GPU)
    "mdc_export_tables": (_i, [_vp, _vp, _sz, _P(_sz)]),
    "mdc_import_tables": (_i, [_vp, _vp, _sz]),
    "mdc_synchronize": (_i, [_vp]),
}
HOST_API = {  # include/mdc_host.h (libmdc_host.so)
    # ---- class UndistorterFOV
    "mdch_fov_create": (_vp, [_cp]),
    "mdch_fov_destroy": (None, [_vp]),
    "mdch_fov_valid": (_i, [_vp]),
    "mdch_fov_has_gpu": (_i, [_vp]),
    "mdch_fov_dims": (None, [_vp, _vp]),
    "mdch_fov_intrinsics": (None, [_vp, _vp]),
    "mdch_fov_remap": (_i, [_vp, _vp, _vp]),
    "mdch_fov_distort": (None, [_vp, _vp, _vp, _i]),
    "mdch_fov_undistort_points": (None, [_vp, _vp, _vp, _i]),
    "mdch_fov_undistort_f32": (None, [_vp, _vp, _vp, _i, _i]),
    "mdch_fov_undistort_u8": (None, [_vp, _vp, _vp, _i, _i]),
    "mdch_fov_model": (None, [_vp, _P(FovModel)]),
    "mdch_fov_lens_model": (_i, [_vp, _P(_i), _P(_f)]),
    "mdch_fov_mdcn_model": (_i, [_vp, _P(LensModel)]),
    # ---- class PhotometricUndistorter
    "mdch_photo_create": (_vp, [_cp, _cp, _i, _i]),
    "mdch_photo_destroy": (None, [_vp]),
    "mdch_photo_valid": (_i, [_vp]),
    "mdch_photo_has_gpu": (_i, [_vp]),
    "mdch_photo_ginv": (_i, [_vp, _vp]),
    "mdch_photo_g": (_i, [_vp, _vp]),
    "mdch_photo_vignette": (_i, [_vp, _vp, _vp]),
    "mdch_photo_unmap": (None, [_vp, _vp, _vp, _i, _i, _i, _i]),
    # ---- tables of the two objects into a GPU context / a blob
    "mdch_bind": (_i, [_vp, _vp, _vp]),
    "mdch_pack_tables": (_i, [_vp, _vp, _vp, _sz, _P(_sz)]),
    # ---- class DatasetReader
    "mdch_reader_create": (_vp, [_cp]),
    "mdch_reader_destroy": (None, [_vp]),
    "mdch_reader_num_images": (_i, [_vp]),
    "mdch_reader_timestamp": (C.c_double, [_vp, _i]),
    "mdch_reader_exposure": (_f, [_vp, _i]),
    "mdch_reader_dims": (None, [_vp, _vp]),
    "mdch_reader_get_image": (_i, [_vp, _i, _i, _i, _i, _i, _vp, C.c_long, _vp, _P(C.c_double), _P(_f)]),
    "mdch_reader_get_images": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, C.c_long, _vp]),
    "mdch_reader_get_images_device": (_i, [_vp, _i, _i, _i, _i, _i, _i, _P(DeviceOutputs), _vp]),
    "mdch_reader_context": (_vp, [_vp]),
    "mdch_reader_device": (_i, [_vp]),
    "mdch_reader_get_raw": (_i, [_vp, _i, _vp, C.c_long, _vp]),
    "mdch_reader_get_images_raw_device": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "mdch_reader_raw_dims": (None, [_vp, _vp]),
    "mdch_reader_set_threads": (None, [_vp, _i]),
    "mdch_reader_set_prefetch": (None, [_vp, _i]),
    "mdch_reader_set_lookahead": (None, [_vp, _i]),
    "mdch_reader_set_gpu_jpeg": (None, [_vp, _i]),
    "mdch_reader_set_gpu_png": (None, [_vp, _i]),
    "mdch_reader_png_device_frames": (C.c_long, [_vp]),
    "mdch_reader_last_error": (_cp, [_vp]),
    "mdch_reader_prefetch_stats": (None, [_vp, _vp]),
    "mdch_reader_device_stats": (_i, [_vp, _i, _vp, _vp]),
    # ---- the reader's frame decoders on a byte string
    "mdch_decode_gray8": (_i, [_vp, _sz, _vp, _sz, _vp, _cp, _sz]),
    "mdch_jpeg_record_bytes": (_sz, [_i, _i, _vp]),
    "mdch_decode_jpeg_record": (_i, [_vp, _sz, _vp, _sz, _i, _vp, _cp, _sz]),
    "mdch_jpeg_stream": (C.c_longlong, [_vp, _sz, _vp, _sz, _vp, _cp, _sz]),
    "mdch_png_stream": (_i, [_vp, _sz, _P(_i), _P(_i), _vp, _sz, _P(_sz)]),
    # ---- ExposureImage's pixel pool
    "mdch_image_alloc": (_vp, [C.c_ulong]),
    "mdch_image_free": (None, [_vp]),
    "mdch_image_pool_trim": (None, []),
    "mdch_image_pool_idle_bytes": (C.c_ulong, []),
}
BENCH_API = {  # include/mdc_bench.h (libmdc_bench.so; not the product ABI)
    "mdcb_synth_frames_device": (_i, [_i, _vp, _i64, _i64, _i, _u32, _vp]),
    "mdcb_ceiling_mix_device": (_i, [_i, _vp, _i64, _vp, _i64, _i, _i, _vp]),
    "mdcb_marker_device": (_i, [_i, _i, _vp]),
    "mdcb_alias_alloc": (_i, [_i, _i64, _i, _P(_vp), _P(_i64)]),
    "mdcb_alias_free": (_i, [_i, _vp, _i64, _i]),
    "mdcb_chunked_alloc": (_i, [_i, _i64, _i, _i, _P(_vp)]),
}
JENC_API = {  # include/mdc_jenc.h (libmdc_jenc.so: the device JPEG encoder, a library of its own)
    "mdcj_jpeg_bound": (_i64, [_i, _i]),
    "mdcj_last_error": (_cp, []),
    "mdcj_create": (_i, [_i, _i, _i, _i, _i, _P(_vp)]),
    "mdcj_destroy": (None, [_vp]),
    "mdcj_encode_f32_device": (_i, [_vp, _vp, _i64, _i, _vp, _i64, _vp, _vp]),
    "mdcj_encode_u8_device": (_i, [_vp, _vp, _i64, _i, _vp, _i64, _vp, _vp]),
    "mdcj_output_device": (_i, [_vp, _P(_vp), _P(_i64), _P(_vp)]),
    "mdcj_fetch": (_i64, [_vp, _vp, _i64, _vp, _i, _vp, _i64, _vp, _vp]),
}
JOPT_API = {  # include/mdc_jopt.h (libmdc_jopt.so: the JPEG encoder with per-frame optimal Huffman tables, a library of its own)
    "mdcjo_jpeg_bound": (_i64, [_i, _i]),
    "mdcjo_last_error": (_cp, []),
    "mdcjo_create": (_i, [_i, _i, _i, _i, _i, _P(_vp)]),
    "mdcjo_destroy": (None, [_vp]),
    "mdcjo_encode_f32_device": (_i, [_vp, _vp, _i64, _i, _vp, _i64, _vp, _vp]),
    "mdcjo_encode_u8_device": (_i, [_vp, _vp, _i64, _i, _vp, _i64, _vp, _vp]),
    "mdcjo_output_device": (_i, [_vp, _P(_vp), _P(_i64), _P(_vp)]),
    "mdcjo_fetch": (_i64, [_vp, _vp, _i64, _vp, _i, _vp, _i64, _vp, _vp]),
    "mdcjo_optimal_tables_device": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "mdcjo_profile": (_i, [_vp, _i]),
    "mdcjo_kernel_ms": (_i, [_vp, _P(_f)]),
}
ZIPW_API = {  # include/mdc_zipw.h (libmdc_zipw.so: ZIP archives of device-resident files, a library of its own)
    "mdcz_last_error": (_cp, []),
    "mdcz_crc_geometry": (None, [_i64, _i64, _P(_i64)]),
    "mdcz_crc32_device": (_i, [_vp, _i64, _vp, _i64, _vp, _vp]),
    "mdcz_crc32_variant_device": (_i, [_i, _vp, _i64, _vp, _i64, _vp, _vp]),
    "mdcz_segment_bound": (_i64, [_i64, _i64, _i]),
    "mdcz_segment_device": (_i, [_vp, _i64, _vp, _vp, _i64, _i64, _cp, _vp, _i64, _vp, _vp]),
    "mdcz_directory": (_i64, [_vp, _i64, _vp, _i64, _i64, _vp, _i64]),
    "mdcz_open": (_i, [_cp, _i, _i64, _P(_vp)]),
    "mdcz_append_device": (_i, [_vp, _vp, _i64, _vp, _vp, _i64, _i64, _cp, _vp]),
    "mdcz_close": (_i64, [_vp]),
    "mdcz_abort": (None, [_vp]),
}
PNGW_API = {  # include/mdc_pngw.h (libmdc_pngw.so: the device PNG encoder, a library of its own on top of libmdc_zipw.so)
    "mdcp_png_bound": (_i64, [_i, _i, _i]),
    "mdcp_last_error": (_cp, []),
    "mdcp_create": (_i, [_i, _i, _i, _i, _i, _i, _P(_vp)]),
    "mdcp_destroy": (None, [_vp]),
    "mdcp_encode_u8_device": (_i, [_vp, _vp, _i64, _i, _vp, _i64, _vp, _vp]),
    "mdcp_encode_u16_device": (_i, [_vp, _vp, _i64, _i, _vp, _i64, _vp, _vp]),
    "mdcp_encode_f32_device": (_i, [_vp, _vp, _i64, _i, _vp, _i64, _vp, _vp]),
    "mdcp_output_device": (_i, [_vp, _P(_vp), _P(_i64), _P(_vp)]),
    "mdcp_huffman_lengths_device": (_i, [_vp, _i, _i, _vp, _vp]),
}
PNGW_RGB_API = {  # include/mdc_pngw_rgb.h (libmdc_pngw_rgb.so: the same encoder built for 8-bit RGB images, a library of its own)
    "mdcp_png_bound_rgb8": (_i64, [_i, _i]),
    "mdcp_last_error_rgb8": (_cp, []),
    "mdcp_create_rgb8": (_i, [_i, _i, _i, _i, _i, _P(_vp)]),
    "mdcp_destroy_rgb8": (None, [_vp]),
    "mdcp_encode_rgb8_device": (_i, [_vp, _vp, _i64, _i, _vp, _i64, _vp, _vp]),
    "mdcp_output_device_rgb8": (_i, [_vp, _P(_vp), _P(_i64), _P(_vp)]),
}
PNGLZ_API = {  # include/mdc_pnglz.h (libmdc_pnglz.so: the PNG encoder with LZ77 matches, gray and RGB, a library of its own)
    "mdcl_png_bound": (_i64, [_i, _i, _i]),
    "mdcl_last_error": (_cp, []),
    "mdcl_create": (_i, [_i, _i, _i, _i, _i, _i, _i, _P(_vp)]),
    "mdcl_destroy": (None, [_vp]),
    "mdcl_encode_u8_device": (_i, [_vp, _vp, _i64, _i, _vp, _i64, _vp, _vp]),
    "mdcl_encode_u16_device": (_i, [_vp, _vp, _i64, _i, _vp, _i64, _vp, _vp]),
    "mdcl_encode_f32_device": (_i, [_vp, _vp, _i64, _i, _vp, _i64, _vp, _vp]),
    "mdcl_encode_rgb8_device": (_i, [_vp, _vp, _i64, _i, _vp, _i64, _vp, _vp]),
    "mdcl_output_device": (_i, [_vp, _P(_vp), _P(_i64), _P(_vp)]),
    "mdcl_form_device": (_i, [_vp, _vp, _i, _vp]),
    "mdcl_profile": (_i, [_vp, _i]),
    "mdcl_kernel_ms": (_i, [_vp, _P(_f)]),
}
PNGD_API = {  # include/mdc_pngd.h (libmdc_pngd.so: the device PNG decoder, a library of its own)
    "mdci_last_error": (_cp, []),
    "mdci_scratch_bytes": (_i64, [_i, _i, _i]),
    "mdci_create": (_i, [_i, _i, _i, _i, _P(_vp)]),
    "mdci_destroy": (None, [_vp]),
    "mdci_decode_device": (_i, [_vp, _vp, _i64, _vp, _i, _i, _i, _vp, _i64, _vp, _vp]),
    "mdci_decode_host": (_i, [_vp, _vp, _vp, _i, _vp, _P(_vp)]),
    "mdci_profile": (_i, [_vp, _i]),
    "mdci_kernel_ms": (_i, [_vp, _P(_f)]),
    "mdci_stream": (_vp, [_vp]),
    "mdci_synchronize": (_i, [_vp]),
}
PNGDX_API = {  # include/mdc_pngdx.h (libmdc_pngdx.so: the device PNG decoder with the parallel inflate, a library of its own)
    "mdcx_last_error": (_cp, []),
    "mdcx_scratch_bytes": (_i64, [_i, _i, _i]),
    "mdcx_create": (_i, [_i, _i, _i, _i, _P(_vp)]),
    "mdcx_destroy": (None, [_vp]),
    "mdcx_decode_device": (_i, [_vp, _vp, _i64, _vp, _i, _i, _i, _vp, _i64, _vp, _vp]),
    "mdcx_decode_host": (_i, [_vp, _vp, _vp, _i, _vp, _P(_vp)]),
    "mdcx_profile": (_i, [_vp, _i]),
    "mdcx_kernel_ms": (_i, [_vp, _P(_f)]),
    "mdcx_stream": (_vp, [_vp]),
    "mdcx_synchronize": (_i, [_vp]),
}
LENS_API = {  # include/mdc_lens.h (libmdc_lens.so: the pinhole / RadTan / EquiDistant lens models on the device, a library of its own)
    "mdcn_last_error": (_cp, []),
    "mdcn_distort_points_device": (_i, [_P(LensModel), _vp, _vp, _i64, _vp]),
    "mdcn_distort_points_host": (_i, [_i, _P(LensModel), _vp, _vp, _i64]),
    "mdcn_remap_device": (_i, [_P(LensModel), _vp, _vp, _vp, _vp]),
}
LENSINV_API = {  # include/mdc_lensinv.h (libmdc_lensinv.so: the lens models run backwards, raw -> rectified, a library of its own)
    "mdcu_last_error": (_cp, []),
    "mdcu_undistort_points_device": (_i, [_P(LensModel), _vp, _vp, _i64, _vp]),
    "mdcu_undistort_points_host": (_i, [_i, _P(LensModel), _vp, _vp, _i64]),
    "mdcu_inverse_remap_device": (_i, [_P(LensModel), _vp, _vp, _vp, _vp]),
}
HIP_SYMBOLS, HOST_SYMBOLS, BENCH_SYMBOLS = list(HIP_API), list(HOST_API), list(BENCH_API)

LIB_BENCH_PATH = os.path.join(_PKG, "libmdc_bench.so")
LIB_JENC_PATH = os.path.join(_PKG, "libmdc_jenc.so")
LIB_JOPT_PATH = os.path.join(_PKG, "libmdc_jopt.so")
LIB_ZIPW_PATH = os.path.join(_PKG, "libmdc_zipw.so")
LIB_PNGW_PATH = os.path.join(_PKG, "libmdc_pngw.so")
LIB_PNGW_RGB_PATH = os.path.join(_PKG, "libmdc_pngw_rgb.so")
LIB_PNGLZ_PATH = os.path.join(_PKG, "libmdc_pnglz.so")
LIB_PNGD_PATH = os.path.join(_PKG, "libmdc_pngd.so")
LIB_PNGDX_PATH = os.path.join(_PKG, "libmdc_pngdx.so")
LIB_LENS_PATH = os.path.join(_PKG, "libmdc_lens.so")
LIB_LENSINV_PATH = os.path.join(_PKG, "libmdc_lensinv.so")
_hip = None
_host = None


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64 (same soname as /opt/rocm's).
    Two HIP runtimes in one process cannot both own the GPU, so when torch is
    installed it must be loaded FIRST: libmdc_hip.so's NEEDED libamdhip64.so.7 then
    resolves to the copy torch already mapped.  Without torch the system runtime
    (RUNPATH /opt/rocm) is used."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def _bind(lib, table, product):
    """The functions of `table` on the loaded library `lib`, each with its restype / argtypes set, as a namespace that holds
    nothing else: a function the table does not declare cannot be called through it (ctypes would marshal its arguments as C
    int).  product: `lib` is the in-tree build, which must have every entry; another build of libmdc_hip (MDC_LIB_HIP, a module
    copy with LIB_HIP_PATH reassigned) may predate some, and those are left out, so that using one raises AttributeError."""
    ns = types.SimpleNamespace()
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name, None)
        if fn is None:
            if product:
                raise OSError("%s does not export %s: rebuild with `python -m mono_dataset_code_amd.build`" % (getattr(lib, "_name", lib), name))
            continue
        fn.restype, fn.argtypes = restype, argtypes
        setattr(ns, name, fn)
    return ns


def _load(path, table, product=True):
    if not os.path.exists(path):
        raise OSError("%s not built: run `python -m mono_dataset_code_amd.build`" % path)
    return _bind(C.CDLL(path), table, product)


def _lazy_lib(path, table, doc):
    """An accessor that loads the library at `path` with the functions of `table` at its first call and returns the same object
    ever after."""
    cache = []

    def lib():
        if not cache:
            _share_hip_runtime_with_torch()
            cache.append(_load(path, table))
        return cache[0]

    lib.__doc__ = doc
    return lib


bench_lib = _lazy_lib(LIB_BENCH_PATH, BENCH_API, "libmdc_bench.so: the synthetic sequence generator and the linear-stream yardstick (bench.py, tools/, tests/).")
jenc_lib = _lazy_lib(LIB_JENC_PATH, JENC_API, "libmdc_jenc.so: the baseline JPEG encoder for device-resident frames (include/mdc_jenc.h).")
jopt_lib = _lazy_lib(LIB_JOPT_PATH, JOPT_API, "libmdc_jopt.so: the JPEG encoder with one optimal Huffman table pair per frame (include/mdc_jopt.h).")
zipw_lib = _lazy_lib(LIB_ZIPW_PATH, ZIPW_API, "libmdc_zipw.so: CRC-32, ZIP segments and the archive writer for device-resident files (include/mdc_zipw.h).")
pngw_lib = _lazy_lib(LIB_PNGW_PATH, PNGW_API, "libmdc_pngw.so: the PNG encoder for device-resident grayscale images (include/mdc_pngw.h).")
pngw_rgb_lib = _lazy_lib(LIB_PNGW_RGB_PATH, PNGW_RGB_API, "libmdc_pngw_rgb.so: the PNG encoder for device-resident 8-bit RGB images (include/mdc_pngw_rgb.h).")
pnglz_lib = _lazy_lib(LIB_PNGLZ_PATH, PNGLZ_API,
                      "libmdc_pnglz.so: the PNG encoder with LZ77 matches for device-resident gray and RGB images (include/mdc_pnglz.h).")
pngd_lib = _lazy_lib(LIB_PNGD_PATH, PNGD_API, "libmdc_pngd.so: the PNG decoder for frames whose zlib streams are in device or host memory (include/mdc_pngd.h).")
pngdx_lib = _lazy_lib(LIB_PNGDX_PATH, PNGDX_API, "libmdc_pngdx.so: the PNG decoder with a parallel inflate for streams with matches (include/mdc_pngdx.h).")
lens_lib = _lazy_lib(LIB_LENS_PATH, LENS_API, "libmdc_lens.so: the pinhole / RadTan / EquiDistant lens models on the device (include/mdc_lens.h).")
lensinv_lib = _lazy_lib(LIB_LENSINV_PATH, LENSINV_API, "libmdc_lensinv.so: raw -> rectified points through every lens model, on the device (include/mdc_lensinv.h).")


def hip_lib():
    global _hip
    if _hip is None:
        _share_hip_runtime_with_torch()
        # LIB_HIP_PATH is read here, not at import: tools/sweep.py and the tests bind module copies to other builds by reassigning it
        _hip = _load(LIB_HIP_PATH, HIP_API, product=LIB_HIP_PATH == os.path.join(_PKG, "libmdc_hip.so"))
    return _hip


def build_flags():
    """Build-time switches of the loaded libmdc_hip.so that are not at their shipped value ("" = the product build)."""
    L = hip_lib()
    return L.mdc_build_flags().decode() if hasattr(L, "mdc_build_flags") else "unknown (library predates mdc_build_flags)"


def code_id():
    """Identity of the loaded libmdc_hip.so's kernel build (hash of sources + flags, include/mdc_hip.h: mdc_code_id)."""
    L = hip_lib()
    return L.mdc_code_id().decode() if hasattr(L, "mdc_code_id") else None


def host_lib():
    global _host
    if _host is None:
        hip_lib()
        _host = _load(LIB_HOST_PATH, HOST_API)
    return _host


def _np_ptr(a):
    return a.ctypes.data_as(_vp) if a is not None else None


def _stream(stream):
    """a hipStream_t given as an integer -> the void* argument (0: the null stream)"""
    return stream if stream else None


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a


class PinnedArray:
    """A numpy view of page-locked host memory (mdc_host_alloc); keep the object alive while the view is used."""

    def __init__(self, shape, dtype):
        self._L = hip_lib()
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._p = self._L.mdc_host_alloc(self.nbytes)
        if not self._p:
            raise MemoryError("mdc_host_alloc(%d) failed" % self.nbytes)
        buf = (C.c_char * self.nbytes).from_address(self._p)
        self.array = np.frombuffer(buf, dtype=dtype).reshape(shape)

    def __del__(self):
        if getattr(self, "_p", None):
            self.array = None
            self._L.mdc_host_free(self._p)
            self._p = None


class Context:
    """One mdc_ctx (one GPU).  Methods map 1:1 onto include/mdc_hip.h."""

    def __init__(self, device=0):
        self._L = hip_lib()
        h = _vp()
        rc = self._L.mdc_create(int(device), C.byref(h))
        if rc != OK:
            raise MdcError(rc, self._L.mdc_last_error(None).decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.mdc_destroy(self._h)
            self._h = None

    __del__ = close

    @property
    def handle(self):
        return self._h

    def _chk(self, rc):
        if rc != OK:
            raise MdcError(rc, self._L.mdc_last_error(self._h).decode())

    def last_error(self):
        return self._L.mdc_last_error(self._h).decode()

    def info(self):
        i = MdcInfo()
        self._chk(self._L.mdc_get_info(self._h, C.byref(i)))
        return i

    def device(self):
        return self.info().device

    def set_option(self, opt, value):
        self._chk(self._L.mdc_set_option(self._h, opt, value))

    def set_photometric(self, ginv, vinv, w, h):
        g = _f32(ginv) if ginv is not None else None
        v = _f32(vinv) if vinv is not None else None
        if g is not None:
            assert g.size == 256
        if v is not None:
            assert v.size == w * h
        self._chk(self._L.mdc_set_photometric(self._h, _np_ptr(g), _np_ptr(v), w, h))

    def set_remap(self, rx, ry, in_w, in_h, out_w, out_h):
        if rx is None:
            self._chk(self._L.mdc_set_remap(self._h, None, None, 0, 0, 0, 0))
            return
        rx, ry = _f32(rx), _f32(ry)
        assert rx.size == out_w * out_h and ry.size == out_w * out_h
        self._chk(self._L.mdc_set_remap(self._h, _np_ptr(rx), _np_ptr(ry), in_w, in_h, out_w, out_h))

    # host-pointer single-frame calls: return the status code, raise only if asked
    def unmap_host(self, img_u8, out_f32, flags, check=True):
        rc = self._L.mdc_unmap_host(self._h, _np_ptr(img_u8), _np_ptr(out_f32), img_u8.size, flags)
        if check:
            self._chk(rc)
        return rc

    def undistort_host(self, img, out_f32, check=True):
        fn = self._L.mdc_undistort_host_f32 if img.dtype == np.float32 else self._L.mdc_undistort_host_u8
        rc = fn(self._h, _np_ptr(img), _np_ptr(out_f32), img.size, out_f32.size)
        if check:
            self._chk(rc)
        return rc

    def process_host(self, raw_u8, out_f32, flags, check=True):
        rc = self._L.mdc_process_host(self._h, _np_ptr(raw_u8), _np_ptr(out_f32), flags)
        if check:
            self._chk(rc)
        return rc

    def process_frames_host(self, raws, outs, flags):
        """raws / outs: sequences of numpy arrays (u8 frames, f32 results), one pair per frame."""
        n = len(raws)
        assert len(outs) == n
        a = (_vp * max(1, n))(*[_np_ptr(r) for r in raws])
        b = (_vp * max(1, n))(*[_np_ptr(o) for o in outs])
        self._chk(self._L.mdc_process_frames_host(self._h, a, b, n, flags))

    def process_jpeg_frames_host(self, records, record_bytes, blocks_w, blocks_rows, outs, flags):
        """records: numpy uint8 arrays (one JPEG coefficient record per frame, decode_jpeg_record), outs: f32 result arrays."""
        n = len(records)
        assert len(outs) == n
        a = (_vp * max(1, n))(*[_np_ptr(r) for r in records])
        b = (_vp * max(1, n))(*[_np_ptr(o) for o in outs])
        self._chk(self._L.mdc_process_jpeg_frames_host(self._h, a, record_bytes, blocks_w, blocks_rows, b, n, flags))

    def process_jpeg_streams_host(self, streams, sizes, outs, flags):
        """streams: numpy uint8 arrays (jpeg_stream), sizes: bytes used of each, outs: f32 result arrays -> per-frame status list."""
        n = len(streams)
        assert len(outs) == n and len(sizes) == n
        a = (_vp * max(1, n))(*[_np_ptr(r) for r in streams])
        b = (_vp * max(1, n))(*[_np_ptr(o) for o in outs])
        sz = (C.c_int64 * max(1, n))(*[int(x) for x in sizes])
        st = (C.c_int * max(1, n))()
        self._chk(self._L.mdc_process_jpeg_streams_host(self._h, a, sz, b, n, flags, st))
        return [int(st[i]) for i in range(n)]

    def process_frames_host_to_device(self, raws, flags, outputs, frame_index=None):
        """raw u8 frames (numpy) -> the device arrays of `outputs` (DeviceOutputs); frame i at position frame_index[i] (None: i)."""
        n = len(raws)
        a = (_vp * max(1, n))(*[_np_ptr(r) for r in raws])
        idx = None if frame_index is None else (C.c_int64 * max(1, n))(*[int(x) for x in frame_index])
        self._chk(self._L.mdc_process_frames_host_to_device(self._h, a, n, flags, C.byref(outputs), idx))

    def process_jpeg_streams_host_to_device(self, streams, sizes, flags, outputs, frame_index=None):
        n = len(streams)
        a = (_vp * max(1, n))(*[_np_ptr(r) for r in streams])
        sz = (C.c_int64 * max(1, n))(*[int(x) for x in sizes])
        idx = None if frame_index is None else (C.c_int64 * max(1, n))(*[int(x) for x in frame_index])
        st = (C.c_int * max(1, n))()
        self._chk(self._L.mdc_process_jpeg_streams_host_to_device(self._h, a, sz, n, flags, C.byref(outputs), idx, st))
        return [int(st[i]) for i in range(n)]

    def jpeg_huffman_batch(self, d_streams, stream_stride, d_records, record_bytes, w, h, blocks_w, blocks_rows, nframes, d_status, stream=0):
        self._chk(self._L.mdc_jpeg_huffman_batch_device(self._h, d_streams, stream_stride, d_records, record_bytes, w, h, blocks_w, blocks_rows,
                                                        nframes, d_status, _stream(stream)))

    def jpeg_idct_batch(self, d_records, record_bytes, d_frames, w, h, blocks_w, blocks_rows, nframes, stream=0):
        self._chk(self._L.mdc_jpeg_idct_batch_device(self._h, d_records, record_bytes, d_frames, w, h, blocks_w, blocks_rows, nframes,
                                                     _stream(stream)))

    # device-pointer batched calls (addresses as ints)
    def unmap_batch(self, d_in, d_out, nframes, flags, stream=0):
        self._chk(self._L.mdc_unmap_batch_device(self._h, d_in, d_out, nframes, flags, _stream(stream)))

    def process_batch(self, d_in, d_out, nframes, flags, stream=0):
        self._chk(self._L.mdc_process_batch_device(self._h, d_in, d_out, nframes, flags, _stream(stream)))

    def undistort_batch_f32(self, d_in, d_out, nframes, stream=0):
        self._chk(self._L.mdc_undistort_batch_device_f32(self._h, d_in, d_out, nframes, _stream(stream)))

    def pyramid_batch(self, d_base, w, h, levels, d_levels, nframes, stream=0):
        arr = (_vp * max(1, len(d_levels)))(*d_levels)
        self._chk(self._L.mdc_pyramid_batch_device(self._h, d_base, w, h, levels, arr, nframes, _stream(stream)))

    def process_pyramid_batch(self, d_in, d_base, levels, d_levels, nframes, flags, stream=0):
        arr = (_vp * max(1, len(d_levels)))(*d_levels)
        self._chk(self._L.mdc_process_pyramid_batch_device(self._h, d_in, d_base, levels, arr, nframes, flags, _stream(stream)))

    def process_pyramid_gradients_batch(self, d_in, d_base, levels, d_levels, d_dI, d_abs, nframes, flags, chunk_frames=0, stream=0):
        """base + levels + (I, dx, dy) / absSquaredGrad of every level in one call; d_dI / d_abs: one address per level (0 = base)."""
        lv = (_vp * max(1, len(d_levels)))(*d_levels)
        di = (_vp * levels)(*d_dI)
        ab = (_vp * levels)(*d_abs)
        self._chk(self._L.mdc_process_pyramid_gradients_batch_device(self._h, d_in, d_base, levels, lv, di, ab, nframes, flags, chunk_frames,
                                                                     _stream(stream)))

    def distort_points_host(self, model, x, y):
        assert x.dtype == np.float32 and y.dtype == np.float32 and x.size == y.size
        self._chk(self._L.mdc_distort_points_host(self._h, C.byref(model), _np_ptr(x), _np_ptr(y), x.size))

    def distort_points_device(self, model, d_x, d_y, n, stream=0):
        self._chk(self._L.mdc_distort_points_device(self._h, C.byref(model), d_x, d_y, n, _stream(stream)))

    def synth_frames(self, d_out, first_frame, nframes, npix, seed, stream=0):
        """(bench / test utility, libmdc_bench.so -- not part of the product ABI)"""
        rc = bench_lib().mdcb_synth_frames_device(self.device(), d_out, first_frame, nframes, npix, seed, _stream(stream))
        if rc != 0:
            raise MdcError(rc, "mdcb_synth_frames_device failed")

    def export_tables(self):
        n = _sz(0)
        self._chk(self._L.mdc_export_tables(self._h, None, 0, C.byref(n)))
        buf = np.zeros(n.value, dtype=np.uint8)
        self._chk(self._L.mdc_export_tables(self._h, _np_ptr(buf), buf.size, C.byref(n)))
        return buf

    def import_tables(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        self._chk(self._L.mdc_import_tables(self._h, _np_ptr(blob), blob.size))

    def synchronize(self):
        self._chk(self._L.mdc_synchronize(self._h))

    def tune_placement(self, d_ins, d_outs, nframes, flags, stream=0):
        """Which PAIR of the candidate input / output buffers (device addresses) does the fused pass run fastest on?  include/mdc_hip.h:
        mdc_tune_placement_device.  -> (best input index, best output index, ms[i][j] for input i with output j)"""
        ni, no = len(d_ins), len(d_outs)
        a, b = (_vp * max(ni, 1))(*d_ins), (_vp * max(no, 1))(*d_outs)
        bi, bo = _i(0), _i(0)
        ms = (C.c_float * max(ni * no, 1))()
        self._chk(self._L.mdc_tune_placement_device(self._h, a, ni, b, no, nframes, flags, _stream(stream), C.byref(bi), C.byref(bo), ms))
        return bi.value, bo.value, [[float(ms[i * no + j]) for j in range(no)] for i in range(ni)]

    def alloc_placed(self, nframes, flags, strategy=PLACE_AUTO, stream=0, in_bytes=0, out_bytes=0):
        """A frame buffer and a result buffer for nframes frames of the pass `flags`, placed by measurement (include/mdc_hip.h:
        mdc_alloc_placed_device).  -> PlacedBuffers; give it back with free_placed()."""
        b = PlacedBuffers()
        self._chk(self._L.mdc_alloc_placed_device(self._h, in_bytes, out_bytes, nframes, flags, strategy, _stream(stream), C.byref(b)))
        return b

    def free_placed(self, b):
        self._chk(self._L.mdc_free_placed_device(self._h, C.byref(b)))

    def alloc_striped_set(self, sizes, stream=0):
        """len(sizes) device buffers, each striped over the device's memory classes (include/mdc_hip.h: mdc_alloc_striped_set_device)
        -> StripedSet (d_ptr[k] = buffer k); give it back with free_striped_set()."""
        b = StripedSet()
        arr = (_sz * len(sizes))(*[int(x) for x in sizes])
        self._chk(self._L.mdc_alloc_striped_set_device(self._h, len(sizes), arr, _stream(stream), C.byref(b)))
        return b

    def free_striped_set(self, b):
        self._chk(self._L.mdc_free_striped_set_device(self._h, C.byref(b)))

    def copy_to_host(self, d_src, count, dtype):
        """count elements of dtype from device address d_src -> numpy array (mdc_copy_to_host: blocking)"""
        out = np.empty(count, dtype=dtype)
        self._chk(self._L.mdc_copy_to_host(self._h, _np_ptr(out), d_src, out.nbytes))
        return out

    def device_alloc(self, nbytes):
        p = _vp()
        self._chk(self._L.mdc_device_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def device_free(self, d_ptr):
        self._L.mdc_device_free(self._h, d_ptr)

    def pci_bus_id(self):
        buf = C.create_string_buffer(32)
        self._chk(self._L.mdc_device_pci_bus_id(self._h, buf, 32))
        return buf.value.decode()

    def describe_launch(self, flags, pyramid_levels=0):
        buf = C.create_string_buffer(256)
        self._chk(self._L.mdc_describe_launch(self._h, flags, pyramid_levels, buf, 256))
        return buf.value.decode()

    def marker(self, ident, stream=0):
        """(bench utility, libmdc_bench.so) a no-op kernel named mdcb_marker_kernel on `stream`: a cut mark in a profiler's kernel trace"""
        if bench_lib().mdcb_marker_device(self.device(), ident, _stream(stream)) != 0:
            raise MdcError(-4, "mdcb_marker_device failed")

    def ceiling_mix(self, d_read, read_bytes, d_write, write_bytes, blocks=16384, span=0, stream=0):
        """(bench utility, libmdc_bench.so -- not part of the product ABI)"""
        rc = bench_lib().mdcb_ceiling_mix_device(self.device(), d_read, read_bytes, d_write, write_bytes, blocks, span, _stream(stream))
        if rc != 0:
            raise MdcError(rc, "mdcb_ceiling_mix_device failed")

    def tune(self, d_in, d_out, nframes, flags, stream=0):
        r = TuneResult()
        self._chk(self._L.mdc_tune_device(self._h, d_in, d_out, nframes, flags, _stream(stream), C.byref(r)))
        return r

    def gradients_batch(self, d_level, w, h, d_dI, d_abs, nframes, stream=0):
        self._chk(self._L.mdc_gradients_batch_device(self._h, d_level, w, h, d_dI, d_abs, nframes, _stream(stream)))

    def vcal_plane_step(self, d_images, d_p2x, d_p2y, d_plane_color, d_vig, oth2, stream=0):
        """torch tensors on the device; d_plane_color is updated in place -> (FF, FC, E, R)."""
        import torch

        n, h, w = d_images.shape
        npnt = d_p2x.shape[1]
        ff = torch.empty(npnt, dtype=torch.float32, device=d_images.device)
        fc = torch.empty_like(ff)
        er = torch.zeros(2, dtype=torch.float64, device=d_images.device)
        self._chk(self._L.mdc_vcal_plane_step_device(self._h, d_images.data_ptr(), d_p2x.data_ptr(), d_p2y.data_ptr(), n, w, h, npnt,
                                                     d_plane_color.data_ptr(), d_vig.data_ptr(), int(oth2), ff.data_ptr(), fc.data_ptr(),
                                                     er.data_ptr(), _stream(stream)))
        e, r = er.cpu().tolist()
        return ff, fc, e, r

    def vcal_vignette_step(self, d_images, d_p2x, d_p2y, d_plane_color, d_vig, oth2, stream=0):
        """d_vig is updated in place -> (TT, CT, E, R)."""
        import torch

        n, h, w = d_images.shape
        npnt = d_p2x.shape[1]
        tt = torch.empty(h * w, dtype=torch.float32, device=d_images.device)
        ct = torch.empty_like(tt)
        er = torch.zeros(2, dtype=torch.float64, device=d_images.device)
        self._chk(self._L.mdc_vcal_vignette_step_device(self._h, d_images.data_ptr(), d_p2x.data_ptr(), d_p2y.data_ptr(), n, w, h, npnt,
                                                        d_plane_color.data_ptr(), d_vig.data_ptr(), int(oth2), tt.data_ptr(), ct.data_ptr(),
                                                        er.data_ptr(), _stream(stream)))
        e, r = er.cpu().tolist()
        return tt, ct, e, r

    def vcal_solve(self, d_images, d_p2x, d_p2y, d_plane_color, d_vig, max_iterations=20, outlier_th=15, stream=0):
        """The reference's whole iteration loop (src/main_vignetteCalib.cpp:395-527); d_plane_color and d_vig are updated
        in place -> array [max_iterations][4] = E, R of the plane step, E, R of the vignette step."""
        n, h, w = d_images.shape
        er = np.zeros((max(max_iterations, 0), 4), np.float64)
        self._chk(self._L.mdc_vcal_solve_device(self._h, d_images.data_ptr(), d_p2x.data_ptr(), d_p2y.data_ptr(), n, w, h, d_p2x.shape[1],
                                                d_plane_color.data_ptr(), d_vig.data_ptr(), int(max_iterations), int(outlier_th),
                                                _np_ptr(er), _stream(stream)))
        return er

    def vcal_scale_images(self, d_images, mean_exposure, d_exposure_times, stream=0):
        """image k = mean_exposure * image k / exposure_time k, in place (src/main_vignetteCalib.cpp:286-291)."""
        n = d_images.shape[0]
        self._chk(self._L.mdc_vcal_scale_images_device(self._h, d_images.data_ptr(), n, d_images[0].numel(), float(mean_exposure),
                                                       d_exposure_times.data_ptr(), _stream(stream)))

    def vcal_gradient_mask(self, d_images, max_abs_grad=255, stream=0):
        """Gradient mask of a stack of calibration images (n, h, w), in place (src/main_vignetteCalib.cpp:293-301)."""
        n, h, w = d_images.shape
        self._chk(self._L.mdc_vcal_gradient_mask_device(self._h, d_images.data_ptr(), n, w, h, int(max_abs_grad), _stream(stream)))

    def vcal_mask_coords(self, d_x, d_y, w, h, stream=0):
        """NaN coordinates for plane points outside the w x h image (src/main_vignetteCalib.cpp:345-357), in place."""
        self._chk(self._L.mdc_vcal_mask_coords_device(self._h, d_x.data_ptr(), d_y.data_ptr(), d_x.numel(), w, h, _stream(stream)))

    def vcal_plane_coords(self, model, gw, gh, facw=5.0, fach=5.0, corners=None, hk=None, stream=0):
        """Plane -> image coordinates of n frames (src/main_vignetteCalib.cpp:230-258, :284, :345-357) -> (p2x, p2y, hk): device
        tensors (n, gw*gh), (n, gw*gh), (n, 3, 3).  corners: (n, 4, 2) float32 device tensor in aruco's corner order (HK is fitted
        from them), or hk: (n, 3, 3) float32 device tensor given as is.  model: FovModel (distortion and coordinate mask) or None
        (the projection only)."""
        import torch

        assert (corners is None) != (hk is None)
        src = corners if hk is None else hk
        n = src.shape[0]
        if hk is None:
            assert corners.dtype == torch.float32 and corners.is_contiguous() and tuple(corners.shape[1:]) == (4, 2)
            hk = torch.empty((n, 3, 3), dtype=torch.float32, device=corners.device)
        assert hk.dtype == torch.float32 and hk.is_contiguous() and tuple(hk.shape) == (n, 3, 3)
        p2x = torch.empty((n, gw * gh), dtype=torch.float32, device=src.device)
        p2y = torch.empty_like(p2x)
        self._chk(self._L.mdc_vcal_plane_coords_device(self._h, C.byref(model) if model is not None else None,
                                                       corners.data_ptr() if corners is not None else None, hk.data_ptr(), n, gw, gh,
                                                       float(facw), float(fach), p2x.data_ptr(), p2y.data_ptr(), _stream(stream)))
        return p2x, p2y, hk

    def vcal_smooth(self, d_vig, w, h, stream=0):
        """vignetteCalib's output smoothing (src/main_vignetteCalib.cpp:541-566) -> (smoothed, scratch) device tensors."""
        import torch

        tt, ct = torch.empty_like(d_vig), torch.empty_like(d_vig)
        self._chk(self._L.mdc_vcal_smooth_device(self._h, d_vig.data_ptr(), w, h, tt.data_ptr(), ct.data_ptr(), _stream(stream)))
        return tt, ct

    def vcal_index(self, d_images, d_p2x, d_p2y, stream=0):
        """Contribution index of the vignette half-iteration for these images / coordinates (mdc_vcal_index_create)."""
        return VcalIndex(self, d_images, d_p2x, d_p2y, stream)

    def vcal_vignette_step_indexed(self, index, d_plane_color, d_vig, oth2, stream=0):
        """The vignette half-iteration as an ordered gather (bit-identical to the reference); d_vig is updated in place
        -> (TT, CT, E, R)."""
        import torch

        tt = torch.empty(index.h * index.w, dtype=torch.float32, device=d_vig.device)
        ct = torch.empty_like(tt)
        er = torch.zeros(2, dtype=torch.float64, device=d_vig.device)
        self._chk(self._L.mdc_vcal_vignette_step_indexed_device(self._h, index._h, d_plane_color.data_ptr(), d_vig.data_ptr(), int(oth2),
                                                                tt.data_ptr(), ct.data_ptr(), er.data_ptr(), _stream(stream)))
        e, r = er.cpu().tolist()
        return tt, ct, e, r

    # ---- responseCalib (include/mdc_hip.h); d_images: (n, h, w) uint8, d_exposure: (n,) float64, d_G: (256,) float64,
    # d_E: (h, w) or (h*w,) float64 -- torch device tensors
    def rcal_leak_pad(self, d_images, leak_padding=2, stream=0):
        """Leak padding (src/main_responseCalib.cpp:208-233), in place."""
        n, h, w = d_images.shape
        self._chk(self._L.mdc_rcal_leak_pad_device(self._h, d_images.data_ptr(), n, w, h, int(leak_padding), _stream(stream)))

    def rcal_init_e(self, d_images, stream=0):
        """Initial irradiance (:250-258) -> E (h*w float64)."""
        import torch

        n, h, w = d_images.shape
        E = torch.empty(h * w, dtype=torch.float64, device=d_images.device)
        self._chk(self._L.mdc_rcal_init_e_device(self._h, d_images.data_ptr(), n, w, h, E.data_ptr(), _stream(stream)))
        return E

    def _rcal_pair(self, d):
        import torch

        return torch.zeros(2, dtype=torch.float64, device=d.device)

    def rcal_rmse(self, d_images, d_exposure, d_G, d_E, stream=0):
        """rmse(G, E) (:50-69) -> (rmse, num)."""
        n, h, w = d_images.shape
        out = self._rcal_pair(d_images)
        self._chk(self._L.mdc_rcal_rmse_device(self._h, d_images.data_ptr(), d_exposure.data_ptr(), n, w, h, d_G.data_ptr(), d_E.data_ptr(),
                                               out.data_ptr(), _stream(stream)))
        a, b = out.cpu().tolist()
        return a, b

    def rcal_g_step(self, d_images, d_exposure, d_E, d_G, stream=0):
        """G step (:285-304), direct (fixed-point) mode; d_G is overwritten."""
        n, h, w = d_images.shape
        self._chk(self._L.mdc_rcal_g_step_device(self._h, d_images.data_ptr(), d_exposure.data_ptr(), n, w, h, d_E.data_ptr(), d_G.data_ptr(),
                                                 _stream(stream)))

    def rcal_index(self, d_images, stream=0):
        """Exact-order index of the stack (mdc_rcal_index_create)."""
        return RcalIndex(self, d_images, stream)

    def rcal_g_step_indexed(self, index, d_exposure, d_E, d_G, stream=0):
        """G step in the reference's order (bit-identical); d_G is overwritten."""
        self._chk(self._L.mdc_rcal_g_step_indexed_device(self._h, index._h, d_exposure.data_ptr(), d_E.data_ptr(), d_G.data_ptr(), _stream(stream)))

    def rcal_e_step(self, d_images, d_exposure, d_G, d_E, stream=0):
        """E step (:319-339), d_E in place -> (rmse, num) of G with the E before the step."""
        n, h, w = d_images.shape
        out = self._rcal_pair(d_images)
        self._chk(self._L.mdc_rcal_e_step_device(self._h, d_images.data_ptr(), d_exposure.data_ptr(), n, w, h, d_G.data_ptr(), d_E.data_ptr(),
                                                 out.data_ptr(), _stream(stream)))
        a, b = out.cpu().tolist()
        return a, b

    def rcal_rescale(self, d_images, d_exposure, d_G, d_E, stream=0):
        """Rescale (:349-356), d_G and d_E in place -> ((rmse, num) before, (rmse, num) after)."""
        n, h, w = d_images.shape
        a, b = self._rcal_pair(d_images), self._rcal_pair(d_images)
        self._chk(self._L.mdc_rcal_rescale_device(self._h, d_images.data_ptr(), d_exposure.data_ptr(), n, w, h, d_G.data_ptr(), d_E.data_ptr(),
                                                  a.data_ptr(), b.data_ptr(), _stream(stream)))
        return tuple(a.cpu().tolist()), tuple(b.cpu().tolist())

    def rcal_solve(self, d_images, d_exposure, iterations=10, mode=RCAL_EXACT_ORDER, stream=0):
        """The whole solve (:250-358) on a leak-padded stack -> (G (256,) float64, E (h*w,) float64 device tensors,
        log dict: init_rmse, init_num, iters = list of per-iteration dicts)."""
        import torch

        n, h, w = d_images.shape
        G = torch.empty(256, dtype=torch.float64, device=d_images.device)
        E = torch.empty(h * w, dtype=torch.float64, device=d_images.device)
        its = (RcalIter * max(int(iterations), 1))()
        lg = RcalLog(0.0, 0.0, C.cast(its, C.POINTER(RcalIter)))
        self._chk(self._L.mdc_rcal_solve_device(self._h, d_images.data_ptr(), d_exposure.data_ptr(), n, w, h, int(iterations), int(mode),
                                                G.data_ptr(), E.data_ptr(), C.byref(lg), _stream(stream)))
        names = [f[0] for f in RcalIter._fields_]
        log = {"init_rmse": lg.init_rmse, "init_num": lg.init_num,
               "iters": [{k: getattr(its[i], k) for k in names} for i in range(int(iterations))]}
        return G, E, log

    def rcal_plot_e(self, d_E, w, h, stream=0):
        """plotE (:72-119) of d_E (w*h float64) -> (rgb (h, w, 3) uint8 in file order R, G, B, e16 (h, w) uint16 (held as int16 bits),
        (Emin, Emax)); synchronises."""
        import torch

        rgb = torch.empty((h, w, 3), dtype=torch.uint8, device=d_E.device)
        e16 = torch.empty((h, w), dtype=torch.int16, device=d_E.device)
        rng = (C.c_double * 2)()
        self._chk(self._L.mdc_rcal_plot_e_device(self._h, d_E.data_ptr(), int(w), int(h), rgb.data_ptr(), e16.data_ptr(), rng, _stream(stream)))
        return rgb, e16, (rng[0], rng[1])

    def rcal_plot_g(self, d_G, stream=0):
        """plotG (:120-146) of d_G (256 float64) -> (img (256, 256) float32 = GImg * 255, (min, max)); synchronises."""
        import torch

        img = torch.empty((256, 256), dtype=torch.float32, device=d_G.device)
        rng = (C.c_double * 2)()
        self._chk(self._L.mdc_rcal_plot_g_device(self._h, d_G.data_ptr(), img.data_ptr(), rng, _stream(stream)))
        return img, (rng[0], rng[1])

    def vcal_plot_plane(self, d_plane, gw, gh, stream=0):
        """displayImage (src/main_vignetteCalib.cpp:72-94) of the gw x gh plane colours (float32) -> (rgb (gh, gw, 3) uint8 in file
        order, (vmin, vmax) as floats); synchronises."""
        import torch

        rgb = torch.empty((gh, gw, 3), dtype=torch.uint8, device=d_plane.device)
        rng = (C.c_float * 2)()
        self._chk(self._L.mdc_vcal_plot_plane_device(self._h, d_plane.data_ptr(), int(gw), int(gh), rgb.data_ptr(), rng, _stream(stream)))
        return rgb, (rng[0], rng[1])

    def vcal_vignette_u16(self, d_vignette, d_out=None, stream=0):
        """The 16-bit pixels of vignette.png / vignetteSmoothed.png (:568-583) of a float32 map -> uint16 values in an int16 tensor of
        the same shape (d_out if given); synchronises."""
        import torch

        if d_out is None:
            d_out = torch.empty(d_vignette.shape, dtype=torch.int16, device=d_vignette.device)
        self._chk(self._L.mdc_vcal_vignette_u16_device(self._h, d_vignette.data_ptr(), d_vignette.numel(), d_out.data_ptr(), _stream(stream)))
        return d_out

    def bind(self, fov=None, photo=None):
        rc = host_lib().mdch_bind(self._h, fov._h if fov is not None else None, photo._h if photo is not None else None)
        self._chk(rc)


class VcalIndex:
    """mdc_vcal_index: per image pixel, the (image, plane point, corner) contributions in the reference's order."""

    def __init__(self, ctx, d_images, d_p2x, d_p2y, stream=0):
        self._L = ctx._L
        self._h = _vp()
        n, self.h, self.w = d_images.shape
        ctx._chk(self._L.mdc_vcal_index_create(ctx._h, d_images.data_ptr(), d_p2x.data_ptr(), d_p2y.data_ptr(), n, self.w, self.h,
                                               d_p2x.shape[1], _stream(stream), C.byref(self._h)))
        self.bytes = self._L.mdc_vcal_index_bytes(self._h)
        self.entries = self._L.mdc_vcal_index_entries(self._h)

    def close(self):
        if self._h:
            self._L.mdc_vcal_index_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RcalIndex:
    """mdc_rcal_index: per byte value, the positions of its samples in the reference's (image, pixel) order."""

    def __init__(self, ctx, d_images, stream=0):
        self._L = ctx._L
        self._h = _vp()
        n, self.h, self.w = d_images.shape
        ctx._chk(self._L.mdc_rcal_index_create(ctx._h, d_images.data_ptr(), n, self.w, self.h, _stream(stream), C.byref(self._h)))
        self.bytes = self._L.mdc_rcal_index_bytes(self._h)
        self.entries = self._L.mdc_rcal_index_entries(self._h)
        self.longest_chain = self._L.mdc_rcal_index_longest_chain(self._h)

    def close(self):
        if self._h:
            self._L.mdc_rcal_index_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_tables(fov=None, photo=None):
    """Host-side table blob (mdch_pack_tables): what rank 0 broadcasts; needs no GPU."""
    L = host_lib()
    n = _sz(0)
    fh = fov._h if fov is not None else None
    ph = photo._h if photo is not None else None
    if L.mdch_pack_tables(fh, ph, None, 0, C.byref(n)) != OK:
        raise MdcError(ERR_ARG, "mdch_pack_tables")
    buf = np.zeros(n.value, dtype=np.uint8)
    if L.mdch_pack_tables(fh, ph, _np_ptr(buf), buf.size, C.byref(n)) != OK:
        raise MdcError(ERR_ARG, "mdch_pack_tables")
    return buf


class UndistorterFOV:
    """Handle on the C++ class UndistorterFOV (include/mono_dataset_code/FOVUndistorter.h)."""

    def __init__(self, camera_txt):
        self._L = host_lib()
        self._h = self._L.mdch_fov_create(os.fsencode(camera_txt))

    def close(self):
        if getattr(self, "_h", None):
            self._L.mdch_fov_destroy(self._h)
            self._h = None

    __del__ = close

    def is_valid(self):
        return bool(self._L.mdch_fov_valid(self._h))

    def has_gpu(self):
        return bool(self._L.mdch_fov_has_gpu(self._h))

    def dims(self):
        d = np.zeros(4, dtype=np.int32)
        self._L.mdch_fov_dims(self._h, _np_ptr(d))
        return tuple(int(x) for x in d)

    def intrinsics(self):
        o = np.zeros(29, dtype=np.float32)
        self._L.mdch_fov_intrinsics(self._h, _np_ptr(o))
        return {"K_rect": o[0:9].reshape(3, 3).copy(), "K_org": o[9:18].reshape(3, 3).copy(),
                "original": o[18:23].copy(), "omega": float(o[23]), "out_calib": o[24:29].copy()}

    def remap(self):
        _, _, ow, oh = self.dims()
        if not self.is_valid():
            return None
        rx = np.zeros(ow * oh, dtype=np.float32)
        ry = np.zeros(ow * oh, dtype=np.float32)
        if not self._L.mdch_fov_remap(self._h, _np_ptr(rx), _np_ptr(ry)):
            return None
        return rx, ry

    def model(self):
        """the FOV model for Context.distort_points_*; raises for a RadTan / EquiDistant camera (the C call gives zeros there)"""
        if self.lens_model()[0] != 0:
            raise MdcError(ERR_ARG, "the camera's lens is %s, which has no FOV model: use mdcn_model()" % LENS_NAMES.get(self.lens_model()[0]))
        m = FovModel()
        self._L.mdch_fov_model(self._h, C.byref(m))
        return m

    def lens_model(self):
        """-> (lensModel(): 0 FOV / pinhole, 1 RadTan, 2 EquiDistant; lensParameters() as 4 floats)"""
        kind, k = _i(0), (_f * 4)()
        self._L.mdch_fov_lens_model(self._h, C.byref(kind), k)
        return kind.value, np.array(k[:], np.float32)

    def mdcn_model(self):
        """the cameras in pixels as a LensModel for capi.Lens; raises where there is none (invalid object, FOV lens with omega != 0)"""
        m = LensModel()
        if not self._L.mdch_fov_mdcn_model(self._h, C.byref(m)):
            raise MdcError(ERR_ARG, "no mdcn_model for this object (invalid, or a FOV lens with omega != 0)")
        return m

    def distort_coordinates(self, x, y):
        assert x.dtype == np.float32 and y.dtype == np.float32 and x.size == y.size
        self._L.mdch_fov_distort(self._h, _np_ptr(x), _np_ptr(y), x.size)

    def undistort_coordinates(self, x, y):
        """undistortCoordinates(): raw pixel coordinates -> rectified ones, in place (NaN where the model cannot bring a point back)"""
        assert x.dtype == np.float32 and y.dtype == np.float32 and x.size == y.size and x.flags.c_contiguous and y.flags.c_contiguous
        self._L.mdch_fov_undistort_points(self._h, _np_ptr(x), _np_ptr(y), x.size)

    def inverse_model(self):
        """the cameras in pixels as a LensModel for capi.LensInverse, of the kind LENSINV_RADTAN / LENSINV_EQUIDISTANT, or LENSINV_FOV
        with k[0] = omega for a FOV / pinhole camera (pixel units by the class's own float and double steps); raises for an invalid
        object"""
        if not self.is_valid():
            raise MdcError(ERR_ARG, "no inverse model for an invalid object")
        if self.lens_model()[0] != 0:
            return self.mdcn_model()  # kinds 1 and 2 keep their values
        f = self.model()
        F, w, h = np.float32, np.float32(f.in_w), np.float32(f.in_h)
        c = [F(v) for v in f.in_calib]
        cam = [c[0] * w, c[1] * h, F(np.float64(c[2] * w) - 0.5), F(np.float64(c[3] * h) - 0.5), c[4], 0, 0, 0]
        o, ow, oh = [F(v) for v in f.out_calib], np.float32(f.out_w), np.float32(f.out_h)
        rect = (o[0] * ow, o[1] * oh, o[2] * ow - F(0.5), o[3] * oh - F(0.5))
        return LensModel.make(LENSINV_FOV, cam, rect, (f.in_w, f.in_h), (f.out_w, f.out_h))

    def undistort(self, img, out):
        fn = self._L.mdch_fov_undistort_f32 if img.dtype == np.float32 else self._L.mdch_fov_undistort_u8
        fn(self._h, _np_ptr(img), _np_ptr(out), img.size, out.size)


class PhotometricUndistorter:
    """Handle on the C++ class PhotometricUndistorter (include/mono_dataset_code/PhotometricUndistorter.h)."""

    def __init__(self, pcalib_txt, vignette_image, w, h):
        self._L = host_lib()
        self.w, self.h = w, h
        self._h = self._L.mdch_photo_create(os.fsencode(pcalib_txt), os.fsencode(vignette_image), w, h)

    def close(self):
        if getattr(self, "_h", None):
            self._L.mdch_photo_destroy(self._h)
            self._h = None

    __del__ = close

    def valid(self):
        return self._L.mdch_photo_valid(self._h)

    def has_gpu(self):
        return bool(self._L.mdch_photo_has_gpu(self._h))

    def ginv(self):
        o = np.zeros(256, dtype=np.float32)
        return o if self._L.mdch_photo_ginv(self._h, _np_ptr(o)) else None

    def g(self):
        o = np.zeros(256, dtype=np.float32)
        return o if self._L.mdch_photo_g(self._h, _np_ptr(o)) else None

    def vignette(self):
        m = np.zeros(self.w * self.h, dtype=np.float32)
        i = np.zeros(self.w * self.h, dtype=np.float32)
        return (m, i) if self._L.mdch_photo_vignette(self._h, _np_ptr(m), _np_ptr(i)) else None

    def unmap(self, img_u8, out_f32, g, v, o):
        self._L.mdch_photo_unmap(self._h, _np_ptr(img_u8), _np_ptr(out_f32), img_u8.size, int(g), int(v), int(o))


class JpegEncoder:
    """One mdcj_encoder (include/mdc_jenc.h): device-resident w x h frames -> one baseline JFIF file per frame, the bytes
    libjpeg writes at `quality`.  huffman="optimal" takes libmdc_jopt.so instead (include/mdc_jopt.h: one Huffman table pair per
    frame, the smaller file libjpeg writes with optimize_coding; the same pixels); "standard", the default, is the Annex K tables.
    encode() fills device slots (the encoder's own unless d_out / d_sizes are given) and returns (d_out, sizes); files() brings
    the encoded bytes, and only those, to the host."""

    def __init__(self, w, h, quality=95, max_frames=1, device=-1, huffman="standard"):
        if huffman not in ("standard", "optimal"):
            raise MdcError(ERR_ARG, "JpegEncoder: huffman %r is neither 'standard' nor 'optimal'" % (huffman,))
        self.huffman = huffman
        self._L = jopt_lib() if huffman == "optimal" else jenc_lib()
        self._prefix = "mdcjo_" if huffman == "optimal" else "mdcj_"
        self.w, self.h, self.quality, self.max_frames = int(w), int(h), int(quality), int(max_frames)
        h_ = _vp()
        self._check(self._fn("create")(int(device), self.w, self.h, self.quality, self.max_frames, C.byref(h_)))
        self._h = h_
        self.bound = int(self._fn("jpeg_bound")(self.w, self.h))
        self._own = None
        self._last = None

    def _fn(self, name):
        return getattr(self._L, self._prefix + name)

    def _check(self, rc):
        if rc < 0:
            raise MdcError(int(rc), self._fn("last_error")().decode())
        return rc

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    __del__ = close

    def output(self):
        """(d_out, slot_bytes, d_sizes): the encoder's own output arrays, max_frames slots of `bound` bytes"""
        if self._own is None:
            o, n, z = _vp(), _i64(), _vp()
            self._check(self._fn("output_device")(self._h, C.byref(o), C.byref(n), C.byref(z)))
            self._own = (o.value, n.value, z.value)
        return self._own

    def encode(self, d_frames, nframes, frame_stride=None, u8=False, d_out=None, slot_bytes=None, d_sizes=None, stream=0):
        """d_frames: device address of nframes float32 (u8: uint8) frames, frame_stride elements apart (default w * h).
        -> (d_out, sizes): the device address of the slots (slot_bytes apart) and the files' lengths as a numpy array."""
        if d_out is None:
            d_out, slot_bytes, d_sizes = self.output()
        fn = self._fn("encode_u8_device" if u8 else "encode_f32_device")
        stride = self.w * self.h if frame_stride is None else int(frame_stride)
        self._check(fn(self._h, d_frames, stride, int(nframes), d_out, int(slot_bytes), d_sizes, _stream(stream)))
        sizes = np.zeros(int(nframes), np.int32)
        self._check(self._fn("fetch")(self._h, d_out, int(slot_bytes), d_sizes, int(nframes), None, 0, _np_ptr(sizes), _stream(stream)))
        self._last = (d_out, int(slot_bytes), d_sizes, int(nframes), stream)
        return d_out, sizes

    def files(self):
        """the files of the last encode() as a list of bytes objects"""
        if self._last is None:
            raise MdcError(ERR_STATE, "JpegEncoder.files: nothing has been encoded")
        d_out, slot_bytes, d_sizes, nframes, stream = self._last
        fetch = self._fn("fetch")
        sizes = np.zeros(nframes, np.int32)
        total = self._check(fetch(self._h, d_out, slot_bytes, d_sizes, nframes, None, 0, _np_ptr(sizes), _stream(stream)))
        buf = np.zeros(max(int(total), 1), np.uint8)
        self._check(fetch(self._h, d_out, slot_bytes, d_sizes, nframes, _np_ptr(buf), buf.size, _np_ptr(sizes), _stream(stream)))
        at = np.concatenate([[0], np.cumsum(sizes)])
        return [buf[at[i]:at[i + 1]].tobytes() for i in range(nframes)]

    def optimal_tables(self, freq, stream=0):
        """huffman="optimal" only: mdcjo_optimal_tables_device on `freq` (ntables x 257 counts, host) -> (bits ntables x 16, vals
        ntables x 256, nvals, status) as numpy arrays; the histograms and results travel through device memory of this call."""
        if self.huffman != "optimal":
            raise MdcError(ERR_STATE, "JpegEncoder.optimal_tables: the encoder was made with huffman='standard'")
        import torch

        freq = np.ascontiguousarray(freq, np.uint32).reshape(-1, 257)
        n = freq.shape[0]
        dev = "cuda:%d" % torch.cuda.current_device()
        d_freq = torch.from_numpy(freq.view(np.int32)).to(dev)
        d_bits, d_vals = torch.zeros(n * 16, dtype=torch.uint8, device=dev), torch.zeros(n * 256, dtype=torch.uint8, device=dev)
        d_nvals, d_status = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
        self._check(self._L.mdcjo_optimal_tables_device(self._h, d_freq.data_ptr(), n, d_bits.data_ptr(), d_vals.data_ptr(), d_nvals.data_ptr(),
                                                        d_status.data_ptr(), _stream(stream)))
        torch.cuda.synchronize()
        return d_bits.cpu().numpy().reshape(n, 16), d_vals.cpu().numpy().reshape(n, 256), d_nvals.cpu().numpy(), d_status.cpu().numpy()


PNG_FILTER_ADAPTIVE = 5  # MDCP_FILTER_ADAPTIVE


class PngEncoder:
    """One mdcp_encoder: device-resident w x h grayscale images of `depth` bits (include/mdc_pngw.h) or, with rgb=True, 8-bit RGB
    images of three bytes R, G, B per pixel (include/mdc_pngw_rgb.h, a library of its own; `depth` is then ignored) -> one PNG
    file per image (filtered, Huffman-only DEFLATE with a stored fallback).  compress="lz77" takes libmdc_pnglz.so instead
    (include/mdc_pnglz.h: the same files with LZ77 matches of depth `chain` where they make a file smaller; all three kinds).
    encode() fills device slots (the encoder's own unless d_out / d_sizes are given) in the layout ZipWriter.append() takes and
    returns their device addresses; it does not synchronise."""

    def __init__(self, w, h, depth=8, filter=PNG_FILTER_ADAPTIVE, max_images=1, device=-1, rgb=False, compress="huffman", chain=4):
        if compress not in ("huffman", "lz77"):
            raise MdcError(ERR_ARG, "PngEncoder: compress %r is neither 'huffman' nor 'lz77'" % (compress,))
        self.rgb, self.lz77, self.chain = bool(rgb), compress == "lz77", int(chain)
        self._L = pnglz_lib() if self.lz77 else pngw_rgb_lib() if self.rgb else pngw_lib()
        L = self._L
        self._prefix = "mdcl_encode_%s_device" if self.lz77 else "mdcp_encode_%s_device"
        self._last_error, self._destroy, self._output = ((L.mdcl_last_error, L.mdcl_destroy, L.mdcl_output_device) if self.lz77 else
                                                         (L.mdcp_last_error_rgb8, L.mdcp_destroy_rgb8, L.mdcp_output_device_rgb8) if self.rgb else
                                                         (L.mdcp_last_error, L.mdcp_destroy, L.mdcp_output_device))
        self.w, self.h, self.depth, self.filter, self.max_images = int(w), int(h), 8 if self.rgb else int(depth), int(filter), int(max_images)
        h_ = _vp()
        if self.lz77:
            if not self.rgb and self.depth not in (8, 16):
                raise MdcError(ERR_ARG, "PngEncoder: depth %d is neither 8 nor 16" % self.depth)
            kind = 2 if self.rgb else 1 if self.depth == 16 else 0  # MDCL_RGB8, MDCL_GRAY16, MDCL_GRAY8
            self._check(L.mdcl_create(int(device), self.w, self.h, kind, self.filter, self.chain, self.max_images, C.byref(h_)))
            self.bound = int(L.mdcl_png_bound(self.w, self.h, kind))
        elif self.rgb:
            self._check(L.mdcp_create_rgb8(int(device), self.w, self.h, self.filter, self.max_images, C.byref(h_)))
            self.bound = int(L.mdcp_png_bound_rgb8(self.w, self.h))
        else:
            self._check(L.mdcp_create(int(device), self.w, self.h, self.depth, self.filter, self.max_images, C.byref(h_)))
            self.bound = int(L.mdcp_png_bound(self.w, self.h, self.depth))
        self._h = h_
        self._own = None

    def _check(self, rc):
        if rc < 0:
            raise MdcError(int(rc), self._last_error().decode())
        return rc

    def close(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    __del__ = close

    def output(self):
        """(d_out, slot_bytes, d_sizes): the encoder's own output arrays, max_images slots of `bound` bytes"""
        if self._own is None:
            o, n, z = _vp(), _i64(), _vp()
            self._check(self._output(self._h, C.byref(o), C.byref(n), C.byref(z)))
            self._own = (o.value, n.value, z.value)
        return self._own

    def encode(self, d_images, nimages, kind=None, stride=None, d_out=None, slot_bytes=None, d_sizes=None, stream=0):
        """d_images: device address of nimages images of `kind` ("u8" (the default), "u16" or "f32"; "rgb8", the only kind and the
        default of an RGB encoder), stride elements apart (default w * h; "rgb8": stride bytes apart, default 3 * w * h).
        -> (d_out, slot_bytes, d_sizes), device addresses."""
        kind = kind or ("rgb8" if self.rgb else "u8")
        if (kind == "rgb8") != self.rgb:
            raise MdcError(ERR_ARG, "PngEncoder.encode: kind %r on %s encoder" % (kind, "an RGB" if self.rgb else "a gray"))
        if d_out is None:
            d_out, slot_bytes, d_sizes = self.output()
        fn = getattr(self._L, self._prefix % kind)
        dense = self.w * self.h * (3 if self.rgb else 1)
        self._check(fn(self._h, d_images, dense if stride is None else int(stride), int(nimages), d_out, int(slot_bytes), d_sizes, _stream(stream)))
        return d_out, int(slot_bytes), d_sizes

    def form_device(self, d_form, nimages, stream=0):
        """compress="lz77" only: four int32 per image of the last encode() call into the device array d_form, on `stream` -- the form
        taken (0 stored, 1 Huffman-only, 2 matches), the parse's tokens, its matches, the match-form stream's bytes"""
        if not self.lz77:
            raise MdcError(ERR_ARG, "PngEncoder.form_device: a Huffman-only encoder has one form")
        self._check(self._L.mdcl_form_device(self._h, d_form, int(nimages), _stream(stream)))

    def profile(self, on=True):
        """compress="lz77" only: HIP events around the stages of every encode() call from now on (kernel_ms reads the last call's)"""
        self._check(self._L.mdcl_profile(self._h, int(bool(on))))

    def kernel_ms(self):
        """-> (filter, order, match, parse, tally, build, scan, pack, finish + checksum) of the last timed call, in ms; waits for it"""
        ms = (_f * 9)()
        self._check(self._L.mdcl_kernel_ms(self._h, ms))
        return tuple(float(v) for v in ms)


PNGD_PATHS = {1: "parallel", 2: "stored", 3: "general"}  # MDCI_PATH_*
PNGDX_PATHS = {1: "parallel", 2: "stored", 3: "general", 4: "tokens"}  # MDCX_PATH_*


class PngDecoder:
    """One mdci_decoder (include/mdc_pngd.h): the zlib streams of w x h 8-bit grayscale PNG frames -> pixels on the device.  A
    status is reason | path << 16 (reason 0: decoded); status_fields() splits an array of them.  matches="parallel": one
    mdcx_decoder (include/mdc_pngdx.h) instead, the same interface with a parallel inflate for streams with matches."""

    def __init__(self, w, h, max_images=1, device=-1, matches="wave"):
        if matches not in ("wave", "parallel"):
            raise ValueError("matches is 'wave' (libmdc_pngd.so) or 'parallel' (libmdc_pngdx.so), not %r" % (matches,))
        self.matches = matches
        self._L, self._prefix = (pngdx_lib(), "mdcx_") if matches == "parallel" else (pngd_lib(), "mdci_")
        self.w, self.h, self.max_images = int(w), int(h), int(max_images)
        h_ = _vp()
        self._check(self._fn("create")(int(device), self.w, self.h, self.max_images, C.byref(h_)))
        self._h = h_
        self.scratch_bytes = int(self._fn("scratch_bytes")(self.w, self.h, self.max_images))

    def _fn(self, name):
        return getattr(self._L, self._prefix + name)

    def _check(self, rc):
        if rc < 0:
            raise MdcError(int(rc), self._fn("last_error")().decode())
        return rc

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    __del__ = close

    def profile(self, on=True):
        """HIP events around the kernels of every decode_device call from now on (kernel_ms reads the last call's)"""
        self._check(self._fn("profile")(self._h, int(bool(on))))

    def kernel_ms(self):
        """-> (front, wave-per-image inflate, checks, unfilter) of the last timed call, in ms; waits for it.  matches="parallel":
        (front, tokens, wave-per-image inflate, checks, unfilter)"""
        ms = (_f * (5 if self.matches == "parallel" else 4))()
        self._check(self._fn("kernel_ms")(self._h, ms))
        return tuple(float(v) for v in ms)

    @staticmethod
    def status_fields(status):
        """-> (reasons, paths) of an array of statuses"""
        s = np.asarray(status, np.int64)
        return s & 0xffff, (s >> 16) & 0xff

    def decode_device(self, d_slots, slot_bytes, d_sizes, n, d_frames, d_status, skip_head=0, skip_tail=0, frame_stride=None, stream=0):
        """device addresses throughout: n slots of slot_bytes, int32 sizes -> frames frame_stride bytes apart (default w * h) and
        int32 statuses; enqueues on `stream` and does not synchronise"""
        self._check(self._fn("decode_device")(self._h, d_slots, int(slot_bytes), d_sizes, int(skip_head), int(skip_tail), int(n), d_frames,
                                               self.w * self.h if frame_stride is None else int(frame_stride), d_status, _stream(stream)))

    def decode_host(self, streams):
        """streams: a list of bytes -> (statuses as an int32 array, the device address of the decoder's dense n x h x w array, valid
        until the next call); blocking"""
        n = len(streams)
        keep = [np.frombuffer(bytes(s), np.uint8) for s in streams]
        ptrs = (_vp * max(n, 1))(*[k.ctypes.data if k.size else None for k in keep])
        sizes = np.asarray([k.size for k in keep], np.int64)
        status = np.zeros(max(n, 1), np.int32)
        d_frames = _vp()
        self._check(self._fn("decode_host")(self._h, ptrs, _np_ptr(sizes) if n else None, n, _np_ptr(status), C.byref(d_frames)))
        return status[:n], d_frames.value


class _LensCalls:
    """What Lens and LensInverse share: one LensModel, and the calls of one library's `_prefix` on it."""

    def __init__(self, model):
        self._L, self.model = self._lib(), model

    def _check(self, rc):
        if rc < 0:
            raise MdcError(int(rc), getattr(self._L, self._prefix + "last_error")().decode())
        return rc

    # the points call (third: n) and the table call (third: the flag's device address) have one shape
    def _device_call(self, name, d_a, d_b, third, stream):
        self._check(getattr(self._L, self._prefix + name)(C.byref(self.model), d_a, d_b, third, _stream(stream)))

    def _host_call(self, name, x, y, device):
        assert x.dtype == np.float32 and y.dtype == np.float32 and x.size == y.size and x.flags.c_contiguous and y.flags.c_contiguous
        self._check(getattr(self._L, self._prefix + name)(int(device), C.byref(self.model), _np_ptr(x), _np_ptr(y), x.size))


class Lens(_LensCalls):
    """The calls of include/mdc_lens.h on one LensModel (UndistorterFOV.mdcn_model(), or LensModel.make)."""
    _lib, _prefix = staticmethod(lens_lib), "mdcn_"

    def distort_points_device(self, d_x, d_y, n, stream=0):
        """n points in the device arrays at d_x, d_y, in place; enqueues on `stream` and does not synchronise"""
        self._device_call("distort_points_device", d_x, d_y, int(n), stream)

    def distort_points_host(self, x, y, device=-1):
        """float32 arrays, in place, blocking; untouched when the call fails (it raises)"""
        self._host_call("distort_points_host", x, y, device)

    def remap_device(self, d_rx, d_ry, d_black, stream=0):
        """the model's out_w x out_h remap tables into device arrays, *d_black (an int32 on the device) = 1 if any entry is black"""
        self._device_call("remap_device", d_rx, d_ry, d_black, stream)


class LensInverse(_LensCalls):
    """The calls of include/mdc_lensinv.h on one LensModel (UndistorterFOV.inverse_model(), or LensModel.make with a LENSINV_* kind)."""
    _lib, _prefix = staticmethod(lensinv_lib), "mdcu_"

    def undistort_points_device(self, d_x, d_y, n, stream=0):
        """n raw points in the device arrays at d_x, d_y -> rectified, in place; enqueues on `stream` and does not synchronise"""
        self._device_call("undistort_points_device", d_x, d_y, int(n), stream)

    def undistort_points_host(self, x, y, device=-1):
        """float32 arrays, in place, blocking; untouched when the call fails (it raises)"""
        self._host_call("undistort_points_host", x, y, device)

    def inverse_remap_device(self, d_ux, d_uy, d_outside, stream=0):
        """the model's in_w x in_h inverse tables into device arrays, *d_outside (an int32 on the device) = 1 if any entry is (-1, -1)"""
        self._device_call("inverse_remap_device", d_ux, d_uy, d_outside, stream)


def huffman_lengths_device(d_hist, nsym, limit, d_lengths, stream=None):
    """mdcp_huffman_lengths_device: the encoder's code builder on nsym uint32 counts -> nsym uint8 lengths (device addresses)"""
    L = pngw_lib()
    if L.mdcp_huffman_lengths_device(d_hist, int(nsym), int(limit), d_lengths, _stream(stream)) < 0:
        raise MdcError(ERR_ARG, L.mdcp_last_error().decode())


ZIPW_RECORD = np.dtype([("offset", "<i8"), ("crc", "<u4"), ("size", "<u4")])  # mdcz_record
ZIPW_NAME_STRIDE = 40  # MDCZ_NAME_STRIDE


def _zipw_check(rc):
    if rc < 0:
        raise MdcError(int(rc), zipw_lib().mdcz_last_error().decode())
    return rc


def crc32_geometry(slot_bytes, nfiles):
    """(bytes per load, a lane's stride, a wave's span, a workgroup's span, parts per file) of the checksum kernel for such a call"""
    out = (_i64 * 5)()
    zipw_lib().mdcz_crc_geometry(int(slot_bytes), int(nfiles), out)
    return tuple(int(v) for v in out)


def crc32_device(d_data, slot_bytes, d_sizes, nfiles, d_crc, stream=None, variant=0):
    """zlib's crc32 of nfiles device-resident byte strings (file f: d_sizes[f] bytes at d_data + f * slot_bytes) into the uint32
    device array d_crc; enqueued on `stream`, not synchronised.  All arguments are device addresses given as integers."""
    L = zipw_lib()
    if variant:
        _zipw_check(L.mdcz_crc32_variant_device(int(variant), d_data, int(slot_bytes), d_sizes, int(nfiles), d_crc, _stream(stream)))
    else:
        _zipw_check(L.mdcz_crc32_device(d_data, int(slot_bytes), d_sizes, int(nfiles), d_crc, _stream(stream)))


def zip_directory(records, names, segment_base_offset=0, directory_offset=0):
    """mdcz_directory on a ZIPW_RECORD array and a list of names (bytes) -> the central directory and end records as bytes"""
    L = zipw_lib()
    records = np.ascontiguousarray(records, dtype=ZIPW_RECORD)
    table = np.zeros((max(len(names), 1), ZIPW_NAME_STRIDE), np.uint8)
    for i, name in enumerate(names):
        if len(name) >= ZIPW_NAME_STRIDE:
            raise MdcError(ERR_ARG, "zip_directory: name %d has %d bytes, at most %d fit" % (i, len(name), ZIPW_NAME_STRIDE - 1))
        table[i, :len(name)] = np.frombuffer(bytes(name), np.uint8)
    n = len(records)
    need = _zipw_check(L.mdcz_directory(_np_ptr(records), n, _np_ptr(table), int(segment_base_offset), int(directory_offset), None, 0))
    out = np.zeros(max(int(need), 1), np.uint8)
    got = _zipw_check(L.mdcz_directory(_np_ptr(records), n, _np_ptr(table), int(segment_base_offset), int(directory_offset), _np_ptr(out), out.size))
    return out[:got].tobytes()


class ZipWriter:
    """One mdcz_writer (include/mdc_zipw.h): an archive of stored entries at `path`, fed with batches of device-resident files.
    append() checksums, lays out and gathers a batch on the device and writes its segment; close() adds the central directory and
    returns the archive's size.  staging_cap (bytes, 0 = the library's default) is where the writer splits a batch."""

    def __init__(self, path, device=0, staging_cap=0):
        self._L = zipw_lib()
        h_ = _vp()
        _zipw_check(self._L.mdcz_open(os.fsencode(path), int(device), int(staging_cap), C.byref(h_)))
        self._h = h_

    def append(self, d_data, slot_bytes, d_sizes, nfiles, first_index=0, suffix=".jpg", valid=None, stream=None):
        """valid: host array of nfiles flags (None = every file); entry names are first_index + f as %05d, then suffix"""
        if not getattr(self, "_h", None):
            raise MdcError(ERR_STATE, "ZipWriter.append: the writer is closed")
        if valid is not None:
            valid = np.ascontiguousarray(valid, dtype=np.uint8)
            if valid.size != int(nfiles):
                raise MdcError(ERR_ARG, "ZipWriter.append: %d flags for %d files" % (valid.size, int(nfiles)))
        sfx = suffix if isinstance(suffix, bytes) else suffix.encode("latin-1")
        _zipw_check(self._L.mdcz_append_device(self._h, d_data, int(slot_bytes), d_sizes, _np_ptr(valid), int(nfiles), int(first_index), sfx, _stream(stream)))

    def close(self):
        """-> the archive's size in bytes (None when already closed)"""
        if getattr(self, "_h", None):
            h_, self._h = self._h, None
            return int(_zipw_check(self._L.mdcz_close(h_)))
        return None

    def abort(self):
        if getattr(self, "_h", None):
            self._L.mdcz_abort(self._h)
            self._h = None

    __del__ = abort


def decode_gray8(data):
    """The reader's frame decoders (8-bit gray PNG, PGM P5, baseline JPEG) on a byte string -> (h, w) uint8 array;
    raises ValueError with the decoder's message."""
    L = host_lib()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    wh = np.zeros(2, np.int32)
    err = C.create_string_buffer(256)
    out = np.zeros(1, np.uint8)
    if not L.mdch_decode_gray8(_np_ptr(buf), buf.size, _np_ptr(out), 0, _np_ptr(wh), err, 256) and (wh[0] <= 0 or wh[1] <= 0):
        raise ValueError(err.value.decode())
    out = np.zeros(int(wh[0]) * int(wh[1]), np.uint8)
    if not L.mdch_decode_gray8(_np_ptr(buf), buf.size, _np_ptr(out), out.size, _np_ptr(wh), err, 256):
        raise ValueError(err.value.decode())
    return out.reshape(int(wh[1]), int(wh[0]))


def jpeg_record_bytes(w, h):
    """-> (record bytes, pitch in blocks, block rows) that fit every sampling layout of a w x h JPEG."""
    pr = np.zeros(2, np.int32)
    n = host_lib().mdch_jpeg_record_bytes(w, h, _np_ptr(pr))
    return int(n), int(pr[0]), int(pr[1])


def decode_jpeg_record(data, record, pitch_blocks):
    """Huffman-decodes a JPEG byte string into `record` (numpy uint8, jpeg_record_bytes long; page-locked for the GPU stage):
    quantisation table + quantised luma coefficients, no inverse DCT.  -> (w, h, pitch_blocks, block rows); ValueError on failure."""
    L = host_lib()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    dims = np.zeros(4, np.int32)
    err = C.create_string_buffer(256)
    if not L.mdch_decode_jpeg_record(_np_ptr(buf), buf.size, _np_ptr(record), record.size, pitch_blocks, _np_ptr(dims), err, 256):
        raise ValueError(err.value.decode())
    return tuple(int(x) for x in dims)


JPEG_STREAM_HEADER_BYTES = 24736


def jpeg_stream(data, stream):
    """Markers parsed, decode tables built, entropy-coded segment unstuffed into `stream` (numpy uint8; page-locked for the GPU
    stage) -> (bytes used, w, h); ValueError for files the device Huffman decoder does not take."""
    L = host_lib()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    wh = np.zeros(2, np.int32)
    err = C.create_string_buffer(256)
    used = L.mdch_jpeg_stream(_np_ptr(buf), buf.size, _np_ptr(stream), stream.size, _np_ptr(wh), err, 256)
    if not used:
        raise ValueError(err.value.decode())
    return int(used), int(wh[0]), int(wh[1])


def png_stream(data, cap=None):
    """The zlib stream (the IDAT bodies, concatenated) of an 8-bit grayscale, non-interlaced PNG file -> (w, h, stream bytes);
    ValueError for every other file and for a stream longer than `cap` (default: the file's length)."""
    L = host_lib()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.zeros(max(buf.size if cap is None else int(cap), 1), np.uint8)
    w, h, used = _i(0), _i(0), _sz(0)
    if not L.mdch_png_stream(_np_ptr(buf) if buf.size else None, buf.size, C.byref(w), C.byref(h), _np_ptr(out), out.size if cap is None else int(cap), C.byref(used)):
        raise ValueError("not a PNG file the device decoder takes")
    return w.value, h.value, out[:used.value].tobytes()


class DatasetReader:
    """class DatasetReader (include/mono_dataset_code/BenchmarkDatasetReader.h) through the C facade."""

    def __init__(self, folder):
        if not folder.endswith("/"):
            folder += "/"
        self._L = host_lib()
        self._h = self._L.mdch_reader_create(os.fsencode(folder))
        d = np.zeros(4, np.int32)
        self._L.mdch_reader_dims(self._h, _np_ptr(d))
        self.in_w, self.in_h, self.out_w, self.out_h = (int(x) for x in d)

    def close(self):
        if getattr(self, "_h", None):
            self._L.mdch_reader_destroy(self._h)
            self._h = None

    __del__ = close

    def __len__(self):
        return self._L.mdch_reader_num_images(self._h)

    def timestamp(self, i):
        return self._L.mdch_reader_timestamp(self._h, i)

    def exposure(self, i):
        return self._L.mdch_reader_exposure(self._h, i)

    def last_error(self):
        return self._L.mdch_reader_last_error(self._h).decode()

    def prefetch_stats(self):
        hm = np.zeros(2, np.int64)
        self._L.mdch_reader_prefetch_stats(self._h, _np_ptr(hm))
        return int(hm[0]), int(hm[1])

    def device_stats(self):
        """Per device the reader deals getImages chunks to (MDC_DEVICES): (device ordinal, frames produced, seconds waiting for
        the decoders, seconds inside the GPU calls), over the reader's life."""
        res = []
        for lane in range(64):
            idf = np.zeros(2, np.int64)
            t = np.zeros(2, np.float64)
            if not self._L.mdch_reader_device_stats(self._h, lane, _np_ptr(idf), _np_ptr(t)):
                break
            res.append((int(idf[0]), int(idf[1]), float(t[0]), float(t[1])))
        return res

    def set_threads(self, n):
        self._L.mdch_reader_set_threads(self._h, n)

    def set_prefetch(self, n):
        self._L.mdch_reader_set_prefetch(self._h, n)

    def set_lookahead(self, frames):
        self._L.mdch_reader_set_lookahead(self._h, int(frames))

    def set_gpu_jpeg(self, stage):
        """True / 2: Huffman decoding + inverse DCT on the GPU; 1: inverse DCT only; False / 0: JPEG decoded on the host."""
        self._L.mdch_reader_set_gpu_jpeg(self._h, (2 if stage else 0) if isinstance(stage, bool) else int(stage))

    def set_gpu_png(self, mode):
        """getImagesDevice on PNG frames.  True / 1: the stream classes that win go to the device decoder; 2: every eligible stream;
        3: every eligible stream through libmdc_pngdx.so (parallel inflate for streams with matches); False / 0: the host decoder."""
        self._L.mdch_reader_set_gpu_png(self._h, int(mode))

    def png_device_frames(self):
        """frames the device PNG decoder has produced for this reader"""
        return int(self._L.mdch_reader_png_device_frames(self._h))

    def get_image(self, i, rectify, g, v, o):
        """-> (image (h, w) float32, timestamp, exposure, id) or None (getImage returned 0)."""
        n = max(self.in_w * self.in_h, self.out_w * self.out_h)
        out = np.empty(n, np.float32)
        meta = np.zeros(3, np.int32)
        ts, ex = C.c_double(0), C.c_float(0)
        if not self._L.mdch_reader_get_image(self._h, i, int(rectify), int(g), int(v), int(o), _np_ptr(out), n, _np_ptr(meta),
                                             C.byref(ts), C.byref(ex)):
            return None
        w, h = int(meta[0]), int(meta[1])
        return out[: w * h].reshape(h, w).copy(), ts.value, ex.value, int(meta[2])

    def get_images(self, first, count, rectify, g, v, o):
        """-> (images (count, h*w) float32, ok mask, number produced)."""
        n = self.out_w * self.out_h if rectify else self.in_w * self.in_h
        out = np.zeros((count, n), np.float32)
        ok = np.zeros(count, np.uint8)
        got = self._L.mdch_reader_get_images(self._h, first, count, int(rectify), int(g), int(v), int(o), _np_ptr(out), n, _np_ptr(ok))
        return out, ok.astype(bool), got

    def get_images_device(self, first, count, rectify, g, v, o, outputs):
        """getImagesDevice: results into the device arrays of `outputs` (DeviceOutputs; frame first + i at position i) -> (valid mask, number produced)."""
        valid = np.zeros(count, np.uint8)
        got = self._L.mdch_reader_get_images_device(self._h, first, count, int(rectify), int(g), int(v), int(o), C.byref(outputs), _np_ptr(valid))
        return valid.astype(bool), got

    def raw_dims(self):
        """getRawSize() -> (w, h)"""
        wh = np.zeros(2, np.int32)
        self._L.mdch_reader_raw_dims(self._h, _np_ptr(wh))
        return int(wh[0]), int(wh[1])

    def get_images_raw_device(self, first, count, step, d_out):
        """getImagesRawDevice: frames first, first+step, ... as u8 into the device tensor d_out (count x w*h bytes, w x h = the
        reader's frame size) -> (valid mask, number delivered)."""
        valid = np.zeros(count, np.uint8)
        got = self._L.mdch_reader_get_images_raw_device(self._h, int(first), int(count), int(step), d_out.data_ptr(), _np_ptr(valid))
        return valid.astype(bool), got

    def device(self):
        return int(self._L.mdch_reader_device(self._h))

    def get_raw(self, i):
        out = np.empty(self.in_w * self.in_h * 4 + 16, np.uint8)
        wh = np.zeros(2, np.int32)
        if not self._L.mdch_reader_get_raw(self._h, i, _np_ptr(out), out.size, _np_ptr(wh)):
            return None
        return out[: int(wh[0]) * int(wh[1])].reshape(int(wh[1]), int(wh[0])).copy()
