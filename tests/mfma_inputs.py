"""Shared by tests/test_mfma_guard.py (GPU) and tests/test_mfma_limbs.py (CPU): the tap-limb model of the int8
MFMA FIR kernels and the comb input that sits in the hole their zero-window guard leaves.

The kernels scale the taps by 2^sc, sc = 14 - ilogb(max|h|), and carry hs = h 2^sc as hi = f16(hs),
lo = f16(hs - hi). With max|hs| >= 2^14, a tap whose second limb is subnormal is kept to 2^-25 absolute in hs,
i.e. to 2^-39 of the largest tap; any other to 2^-22 of itself. The int8 samples are exact in f16 and the
products exact in the fp32 accumulator, so beyond the fp32 accumulation (inside the 1e-6 sum|h||x| contract) an
output's error is at most LIMB_FLOOR max|h| sum_j |x[kD + j]|."""
import numpy as np

LIMB_REL = 2.0 ** -22    # per tap, of itself
LIMB_FLOOR = 2.0 ** -39  # per tap, of the largest tap


def limb_split(taps):
    """(hi + lo) 2^-sc in float64: the taps as the MFMA kernels carry them."""
    h = np.asarray(taps, np.float32)
    peak = float(np.max(np.abs(h)))
    sc = 14 - (int(np.frexp(peak)[1]) - 1) if peak > 0 else 0  # ilogb = frexp's exponent - 1
    hs = np.ldexp(h, sc).astype(np.float32)  # a power of two: exact
    with np.errstate(under="ignore"):
        hi = hs.astype(np.float16)
        lo = (hs - hi.astype(np.float32)).astype(np.float16)
    return np.ldexp(hi.astype(np.float64) + lo.astype(np.float64), -sc)


# (T, D, cutoff, window, n_out, engineered outputs): first and last outputs of 512-output tiles, one inside a
# later tile; C2 also at output indices past 4096. At these sizes every block of a launch owns one tile, so
# the indices pick tiles and positions inside a tile, not a block's later tiles or second chunk (those:
# test_mfma_guard.py::test_int8_mfma_gaps_in_later_tiles). Windows at least ceil(T / D) + 1 outputs apart.
COMB_C2 = [(127, 1, 0.1, "hamming", 10_000, (0, 1023, 1536, 2600, 4396, 5119, 9216)),
           (127, 1, 0.1, "blackman", 10_000, (0, 1023, 1536, 2600, 4396, 5119, 9216))]
COMB_DEC = [(255, 5, 0.1, "blackman", 4000, (512, 1023, 1736, 2047, 3072, 3900)),
            (1023, 10, 0.1, "blackman", 4000, (512, 1023, 1736, 2047, 3072, 3900))]


def comb_iq(T, D, cut, n_out, k0s, seed=0xC0B):
    """int8 IQ with no zero component, except inside the window of each engineered output k0: there only the
    samples under the sinc's zeros (tap index = centre mod period, the centre itself excluded) stay non-zero."""
    p = int(round(1.0 / (2.0 * cut)))
    assert abs(p - 1.0 / (2.0 * cut)) < 1e-9 and T % 2 == 1 and len(k0s) <= 8
    c = (T - 1) // 2
    n_in = (n_out - 1) * D + T
    rng = np.random.default_rng(seed)
    iq = rng.integers(-128, 128, 2 * n_in).astype(np.int8)
    iq[iq == 0] = 1
    j = np.arange(T)
    gone = (j % p != c % p) | (j == c)
    ks = sorted(k0s)
    assert all(b - a >= -(-T // D) + 1 for a, b in zip(ks, ks[1:])) and ks[-1] < n_out
    for k0 in ks:
        win = iq[2 * k0 * D: 2 * (k0 * D + T)].reshape(T, 2)
        win[gone] = 0
    return iq


def longest_zero_run(iq):
    """Longest run of exact-zero complex samples in interleaved int8 IQ."""
    z = (iq.reshape(-1, 2) == 0).all(axis=1).astype(np.int8)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], z, [0]])))
    return int((edges[1::2] - edges[::2]).max()) if edges.size else 0


def window_abs_sum(xc, T, D, n_out):
    """sum_j |x[kD + j]| per output k (float64), for the limb floor."""
    cs = np.concatenate([[0.0], np.cumsum(np.abs(xc.astype(np.complex128)))])
    k = np.arange(n_out) * D
    return cs[k + T] - cs[k]
