"""Grid spacings at which dx * d, 1 / (2 dx) and (pe - pw) * two_dx_inv are all INEXACT products.

With a power-of-two dx every product that depends on the spacing is exact, so a contracted fmaf(dx, d, -sum), a contracted
fmaf(-(pe - pw), two_dx_inv, u) or a division by 2 dx in place of the multiplication by its reciprocal leave the reference's
bits.  At the spacings below each of these changes a few per cent of the cells after one operator.  Every value is a
float32: it reaches the oracle, the reference and the library as the same number.
"""
import numpy as np

DX_A = np.float32(0.37)                                   # the spacing of the views' tests
DX_B = np.float32(1.37)
DX_C = np.float32(3.0)                                    # 2 dx exact, the reciprocal inexact
DX_D = np.float32(0.1)
DX_E = np.nextafter(np.float32(1), np.float32(2))         # the smallest dx that must not take the kernels compiled for dx = 1

DX_CASES = (DX_A, DX_B, DX_C, DX_D, DX_E)
DX_TAGS = ("a", "b", "c", "d", "e")                      # the names of the spacings in the dxn_ fixtures


def dx_id(dx):
    """A pytest id: nextafter(1) prints as 1.0000001."""
    return f"dx{float(np.float32(dx)):.8g}"


def widened(dx):
    """The float32 as a Python float: the same number for every float32 consumer, and a literal a sequence can print."""
    return float(np.float32(dx))
