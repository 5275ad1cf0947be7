"""Cases of the shell spectra and spectral transfers of the periodic spectral solver: the five shapes of tests/pspec_scalar_cases.py with their
full-band flow, scalar, Kolmogorov force and drag (tests/test_gpu_pspec_spectrum.py runs them on the GPU against tests/pspec_spectrum_oracle.py;
tests/test_oracle_pspec_spectrum.py shows on the CPU that their bounds would catch a wrong shell rule, weight, shell width, a missing 1 / |k|^2,
a sign flip of the nonlinear term and a mean gradient left in the scalar's transfer)."""
import pspec_scalar_cases as SC
import pspec_spectrum_oracle as PO

# 64x64x3 with a mean flow, 128x512x2 and 512x128x2 with both boxes != 2 pi, 1024x64x2, 64x1024x2: both partial column tiles, the 4-line tiles of
# N = 1024 on each axis, nx != ny; S = 31, 240, 346, 343, 343 shells
CASES = SC.CASES
NSTEPS = SC.NSTEPS
reference = SC.reference

# The GPU's shell sums against the restatement's sums over the SAME float32 spectrum, both in float64: only the order of summation differs.
# A shell holds <= ~7000 terms, each rounded to 2^-53 relative: 7000 * 1.1e-16 = 8e-13 in the worst case of errors all of one sign; bound 1e-11.
BOUND_SPECTRUM = 1e-11

# The GPU's transfers (one float32 evaluation of the nonlinear term, summed in float64) against the restatement's of the same state:
# sum_s |T_gpu - T_oracle| / sum_s A(s) for T_E, T_Z, T_theta, then |sum_s T_gpu| / sum_s A(s) for the three, then the energy budget on its
# own scale.  Measured on the MI355X (worst grid of the batch):
#   64x64    1.79e-07 2.77e-08 4.55e-08 | 1.56e-07 9.28e-09 1.89e-08 | 3.99e-08
#   128x512  1.20e-07 2.23e-08 3.81e-08 | 4.10e-08 5.13e-10 4.02e-09 | 5.75e-08
#   512x128  1.37e-07 2.79e-08 4.88e-08 | 1.36e-08 1.52e-09 7.86e-09 | 5.08e-08
#   1024x64  2.24e-07 4.91e-08 6.22e-08 | 3.01e-08 1.75e-09 7.76e-09 | 2.73e-08
#   64x1024  5.80e-07 1.28e-07 1.45e-07 | 2.74e-08 9.06e-09 1.28e-08 | 3.45e-08
# Worst 5.80e-7 (T_E at 64x1024: the 1 / |k|^2 weights the few largest scales, where the absolute float32 error of a 1024-point transform is
# largest against the mode's own size); bound 2e-6 = 3.4x, the margin of pspec_cases.BOUND_UV.  The wrong definitions of
# tests/test_oracle_pspec_spectrum.py move the same measures by >= 2.2e-2, 10000x the bound.
BOUND_TRANSFER = 2e-6

# no kept mode of any case may sit on a shell boundary: there the float64 rounding of |k| / dk + 1/2, not the definition, would pick the side
BOUNDARY_DISTANCE = {}
for _c in CASES:
    _nx, _ny, _B, _Lx, _Ly, _ = _c
    BOUNDARY_DISTANCE[_c[:2]] = PO.boundary_distance(SC.scheme(_nx, _ny, 1.0, _Lx, _Ly, forced=False))
    assert BOUNDARY_DISTANCE[_c[:2]] >= 1e-9, (_c, BOUNDARY_DISTANCE[_c[:2]])


def spectra_of(case, w, t):
    """(scheme, spectrum dict, transfer dict) of the restatement for the state (w, t) [B, nx, nh] of a case, under the case's force and drag."""
    nx, ny, B, Lx, Ly, _ = case
    S = SC.reference(case)[0]
    return S, PO.spectrum(S, w, t), PO.transfer(S, w, t)
