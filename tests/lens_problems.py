"""The cameras tests/test_lens_cpu.py and tests/test_lens.py run: name -> the four lines of camera.txt."""

SMALL_IN, SMALL_OUT = "96 80", "64 48"
BARREL = "RadTan 60 58 47.5 39.5 -0.25 0.06 0.001 -0.0005"  # barrel with tangential terms
PINCUSHION = "RadTan 60 58 47.5 39.5 0.12 0.01 0 0"  # 26 crop rounds
FISHEYE = "EquiDistant 40 40 47.5 39.5 0.01 -0.003 0.001 0"
EUROC = "RadTan 458.654 457.296 367.215 248.375 -0.28340811 0.07395907 0.00019359 1.76187114e-05"
TUMVI = "EquiDistant 190.978 190.973 254.931 256.897 0.003482389 0.000715034 -0.002053236 0.000202936"

# the three small cameras: `crop`, and one explicit line 3 each (the pincushion one chosen so that the corners go black)
SMALL = {
    "barrel_crop": (BARREL, SMALL_IN, "crop", SMALL_OUT),
    "pincushion_crop": (PINCUSHION, SMALL_IN, "crop", SMALL_OUT),
    "fisheye_crop": (FISHEYE, SMALL_IN, "crop", SMALL_OUT),
    "barrel_explicit": (BARREL, SMALL_IN, "0.62 0.70 0.5 0.5 0", SMALL_OUT),
    "pincushion_explicit_black": (PINCUSHION, SMALL_IN, "0.45 0.5 0.5 0.5 0", SMALL_OUT),
    "fisheye_explicit": (FISHEYE, SMALL_IN, "0.30 0.40 0.48 0.52 0", SMALL_OUT),
}
CROP_ROUNDS = {"barrel_crop": 4, "pincushion_crop": 26, "fisheye_crop": 4, "euroc": 4, "tumvi": 4}

# the same three in relative units (fx / 96, fy / 80, (cx + 0.5) / 96, (cy + 0.5) / 80), KannalaBrandt spelled out, a width that is
# no multiple of 16 (the gather kernel), and the two public cameras at full size
MORE = {
    "barrel_relative": ("RadTan 0.625 0.725 0.5 0.5 -0.25 0.06 0.001 -0.0005", SMALL_IN, "crop", SMALL_OUT),
    "pincushion_relative": ("RadTan 0.625 0.725 0.5 0.5 0.12 0.01 0 0", SMALL_IN, "crop", SMALL_OUT),
    "fisheye_relative": ("EquiDistant 0.41666666 0.5 0.5 0.5 0.01 -0.003 0.001 0", SMALL_IN, "crop", SMALL_OUT),
    "kannala_brandt": (FISHEYE.replace("EquiDistant", "KannalaBrandt"), SMALL_IN, "crop", SMALL_OUT),
    "barrel_ragged": ("RadTan 62 58 48.5 39.5 -0.25 0.06 0.001 -0.0005", "99 80", "crop", "61 47"),
}
FULL = {
    "euroc": (EUROC, "752 480", "crop", "640 480"),
    "tumvi": (TUMVI, "512 512", "crop", "512 512"),
}
PROBLEMS = dict(SMALL, **MORE, **FULL)

HEADER_MESSAGE = "Failed to read camera calibration (invalid format?)"
# name -> (lines, the message the object prints, whether getInputDims still answers)
MALFORMED = {
    "seven_parameters": (("RadTan 60 58 47.5 39.5 -0.25 0.06 0.001", SMALL_IN, "crop", SMALL_OUT), HEADER_MESSAGE, False),
    "nan": (("RadTan 60 58 47.5 39.5 nan 0.06 0.001 -0.0005", SMALL_IN, "crop", SMALL_OUT), HEADER_MESSAGE, False),
    "fx_zero": (("EquiDistant 0 40 47.5 39.5 0.01 -0.003 0.001 0", SMALL_IN, "crop", SMALL_OUT), HEADER_MESSAGE, False),
    "full": ((BARREL, SMALL_IN, "full", SMALL_OUT), "Out: Full is not implemented for this lens model... not rectifying.", True),
    "crop_one_wide": ((BARREL, SMALL_IN, "crop", "1 48"), "Out: Crop needs an output of at least 2 x 2 pixels... not rectifying.", True),
}


def write_camera(folder, lines):
    import os

    path = os.path.join(str(folder), "camera.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path
