"""vignetteCalib's plane -> image coordinates, the product side that needs no GPU: mdc_vcal_plane_coords_device is declared, exported and
wrapped, and its kernels compile without scratch.  (The arithmetic is checked on the device, tests/test_vcal_plane_coords.py.)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_and_exported():
    from mono_dataset_code_amd import capi

    assert "mdc_vcal_plane_coords_device" in open(os.path.join(ROOT, "include", "mdc_hip.h")).read()
    assert "mdc_vcal_plane_coords_device" in capi.HIP_SYMBOLS
    L = capi.hip_lib()
    assert hasattr(L, "mdc_vcal_plane_coords_device")
    assert hasattr(capi.Context, "vcal_plane_coords")


def test_plane_coords_kernels_use_no_scratch():
    """The new kernels of mdc_vcal.hip: no scratch, and their register counts (a lane per frame for the homography, a lane per
    plane point for the coordinates: neither is near an occupancy limit)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    ks = {k["pretty"]: k for k in isa_stats.kernels(isa_stats.device_asm("mdc_vcal.hip"))}
    names = ["vcal_plane_homography_kernel", "vcal_plane_coords_kernel<true>", "vcal_plane_coords_kernel<false>"]
    for n in names:
        assert n in ks, sorted(ks)
        assert ks[n]["scratch"] == 0, (n, ks[n]["scratch"])
        assert ks[n]["vgpr"] <= 64, (n, ks[n]["vgpr"])
        assert not any(m.startswith("v_mfma") for m in ks[n]["counts"]), n
    print({n: (ks[n]["vgpr"], ks[n]["sgpr"]) for n in names})
