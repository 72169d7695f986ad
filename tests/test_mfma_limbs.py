"""The tap-limb model of the int8 MFMA FIR kernels, on the CPU (no GPU needed).

tests/test_mfma_guard.py::test_int8_mfma_comb_under_sinc_zeros bounds the kernels' error on the comb input by
1e-6 sum|h||x| + 2^-39 max|h| sum|x|. That floor rests on the limb split (mfma_inputs.limb_split restates the
kernels' arithmetic: fir_i8_mfma.hip, fir_cf_mfma.hip), so the split is pinned here for the project's filters,
and the comb generator is checked against the emulation: exactly the engineered outputs leave the 1e-6 bound,
none leaves the floor."""
import numpy as np
import pytest

import mfma_inputs as mi

FIR_TOL = 1e-6

FILTERS = [(127, 0.1, "hamming"), (127, 0.1, "blackman"), (129, 0.1, "blackman"), (33, 0.1, "blackman"),
           (1023, 0.04, "blackman"), (255, 0.08, "blackman"), (640, 0.025, "blackman"), (255, 0.1, "blackman"),
           (1023, 0.1, "blackman")]


@pytest.mark.parametrize("T,cut,window", FILTERS)
def test_tap_limbs_keep_each_tap(orc, T, cut, window):
    """|hi + lo - hs| 2^-sc <= max(2^-22 |h_j|, 2^-39 max|h|) for every tap."""
    h = orc.lowpass_taps(T, cut, window).astype(np.float64)
    err = np.abs(mi.limb_split(h) - h)
    lim = np.maximum(mi.LIMB_REL * np.abs(h), mi.LIMB_FLOOR * np.max(np.abs(h)))
    bad = np.nonzero(~(err <= lim))[0]
    assert bad.size == 0, [(int(j), float(h[j]), float(err[j] / lim[j])) for j in bad[:8]]
    # the model is not vacuous: these filters do have taps the limbs lose completely
    assert np.any((mi.limb_split(h) == 0) & (h != 0))


def test_limb_split_examples():
    """Hand-checked values: peak 1 -> sc = 14; 2^-25 of the peak is half the smallest subnormal f16 step."""
    h = np.array([1.0, 1.0 + 2.0 ** -20, 2.0 ** -39, 2.0 ** -40, 3.0 * 2.0 ** -39, 1e-17, 0.0], np.float32)
    q = mi.limb_split(h)
    assert q[0] == 1.0 and q[1] == 1.0 + 2.0 ** -20 and q[6] == 0.0
    assert q[2] in (0.0, 2.0 ** -38)        # hs = 2^-25: a tie between 0 and the first subnormal
    assert q[3] == 0.0 and q[5] == 0.0      # below half a step: lost
    assert abs(q[4] - 3.0 * 2.0 ** -39) <= mi.LIMB_FLOOR
    assert np.array_equal(mi.limb_split(np.ldexp(h, -9)), np.ldexp(q, -9))  # the block scale follows the peak


@pytest.mark.parametrize("T,D,cut,window,n_out,k0s", mi.COMB_C2 + mi.COMB_DEC)
def test_comb_input_on_the_emulated_limbs(orc, T, D, cut, window, n_out, k0s):
    """The comb generator against the emulation: no zero run the guard could flag (<= 15 samples), exactly the
    engineered outputs outside 1e-6 sum|h||x|, every output inside the bound plus the limb floor."""
    iq = mi.comb_iq(T, D, cut, n_out, k0s)
    assert mi.longest_zero_run(iq) <= 15
    taps = orc.lowpass_taps(T, cut, window)
    xc = orc.int8_to_float(iq).view(np.complex64)
    _, bound = orc.fir_f64(taps, xc, D, n_out)
    dh = mi.limb_split(taps) - taps.astype(np.float64)
    win = np.lib.stride_tricks.sliding_window_view(xc, T)[::D][:n_out]
    err = np.abs(win.astype(np.complex128) @ dh)
    outside = np.nonzero(~(err <= FIR_TOL * bound))[0]
    assert outside.tolist() == sorted(k0s), (outside[:12].tolist(), sorted(k0s))
    floor = mi.LIMB_FLOOR * float(np.max(np.abs(taps))) * mi.window_abs_sum(xc, T, D, n_out)
    worst = err / (FIR_TOL * bound + floor)
    assert np.all(worst <= 1.0), (int(np.argmax(worst)), float(worst.max()))
