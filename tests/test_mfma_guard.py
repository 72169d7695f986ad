"""The matrix-core FIR kernels on adversarial inputs (r06).

The MFMA kernels multiply f16 limbs: the taps as two limbs under one block scale (hi + lo, each tap kept to
2^-22 of itself only while it lies within ~2^-17 of the largest tap), the cf32 samples as two limbs under a
per-tile scale. A window whose non-zero samples all sit under taps below that range - a Blackman filter's
tails at a zero-padded stream start, after an exact-zero gap, between sparse impulses - loses its output,
which the 1e-6 sum|h||x| bound does not allow. Each kernel therefore computes such tiles in
the direct form: the cf32 kernels send a tile with an exact-zero 64-sample block to their direct path
(the guard already sent quiet blocks there), the int8 kernels a tile whose window holds an exact-zero run.

Every MFMA route is run here against float64 per element, complex and AM outputs:
  cf32   the FFT kernel's adversarial signals (tests/test_fft_fir.py) on the wave-specialised f16 kernel, the
         synchronous f16 kernel (GSDR_POLICY_NO_WS) and the bf16 x 3 kernel (GSDR_POLICY_CF_BF16);
  int8   zero-padded starts, exact-zero gaps, burst onsets and all-zero streams on C2's kernel (D = 1, S = 2
         and S = 5, Hamming and Blackman), the 4-way, 8-way (GSDR_POLICY_I8_WS8) and synchronous
         (GSDR_POLICY_NO_WS, and by shape at D = 16) decimating kernels, and the fused chain on the 4-way and
         8-way kernels; and many-gap streams in launches large enough that every block of the two kernels with
         per-tile guard state in LDS (C2, synchronous) walks several tiles and chunks.
What no guard catches - a comb whose non-zero samples sit only under a windowed sinc's zeros, which holds no
zero run - is pinned by test_int8_mfma_comb_under_sinc_zeros: there the error may leave the 1e-6 bound, but
only by the limbs' floor, 2^-39 max|h| sum|x| (tests/mfma_inputs.py, tests/test_mfma_limbs.py).
Reference arithmetic: Fir.cpp:229-269 (gsdrFirFC)."""
import functools

import numpy as np
import pytest

import mfma_inputs as mi

pytestmark = pytest.mark.gpu

FIR_TOL = 1e-6


@pytest.fixture(scope="module")
def ops():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpusdr import ops
    return ops


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()  # the shared cases are read-only


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


class _Policy:
    """`flags`: a policy word, or the names of ops.POLICY_* flags (parametrised cases name them)."""

    def __init__(self, ops, flags):
        if not isinstance(flags, int):
            flags = functools.reduce(lambda acc, name: acc | getattr(ops, "POLICY_" + name), flags, 0)
        self.ops, self.flags = ops, flags

    def __enter__(self):
        self.prev = self.ops.set_kernel_policy(self.flags)

    def __exit__(self, *exc):
        self.ops.set_kernel_policy(self.prev)


def _check(y, y64, bound, what, tile_out=512):
    err = np.abs(y.astype(np.complex128) - y64)
    bad = np.nonzero(~(err <= FIR_TOL * bound + 1e-30))[0]
    assert bad.size == 0, (what, int(bad.size), [(int(k), int(k // tile_out), float(err[k] / (bound[k] + 1e-300)))
                                                 for k in bad[:8]])


def _adversarial(name, n, rng):
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    i = np.arange(n)
    if name == "silence":
        x[(i // 7000) % 3 == 1] = 0
    elif name == "impulses":
        x = np.zeros(n, np.complex64)
        x[::997] = 1 + 1j
    elif name == "zero-start":
        x[: 5000] = 0
    return x


@pytest.mark.parametrize("name", ["silence", "impulses", "zero-start"])
@pytest.mark.parametrize("T,D,window", [(1023, 10, "blackman"), (200, 3, "blackman")])
def test_cf_mfma_adversarial(ops, orc, name, T, D, window):
    """cf32 x real taps on the wave-specialised f16 MFMA kernel (T = 200, D = 3 takes it by default: the
    FFT kernel needs D in {1, 2, 4, 6, 8, 10}; C3's shape under GSDR_POLICY_NO_FFT)."""
    n_out = 40_000
    n_in = (n_out - 1) * D + T
    x = _adversarial(name, n_in, np.random.default_rng(11))
    taps = orc.lowpass_taps(T, 0.4 / D, window)
    x_d, taps_d = _dev(x), _dev(taps)
    with _Policy(ops, ops.POLICY_NO_FFT):
        assert ops.fir_kernel_class(x_d, taps_d, D) == "cf-mfma"
        y = _host(ops.fir(taps_d, x_d, D, n_out))
        am = _host(ops.fir(taps_d, x_d, D, n_out, am=True))
    y64, bound = orc.fir_f64(taps, x, D, n_out)
    _check(y, y64, bound, ("cf-mfma", name, T, D))
    _check(am, np.abs(y64), bound, ("cf-mfma-am", name, T, D))


@functools.lru_cache(maxsize=None)
def _cf_case(name, T, D, window):
    """The adversarial cf32 case and its float64 reference, shared by the routes (read only)."""
    import oracle as orc
    n_out = 40_000
    x = _adversarial(name, (n_out - 1) * D + T, np.random.default_rng(11))
    taps = orc.lowpass_taps(T, 0.4 / D, window)
    y64, bound = orc.fir_f64(taps, x, D, n_out)
    for a in (x, taps, y64, bound):
        a.setflags(write=False)
    return x, taps, n_out, y64, bound


@pytest.mark.parametrize("name", ["silence", "impulses", "zero-start"])
@pytest.mark.parametrize("T,D,window", [(1023, 10, "blackman"), (200, 3, "blackman")])
@pytest.mark.parametrize("route,flags", [("sync-f16", ("NO_FFT", "NO_WS")), ("bf16x3", ("NO_FFT", "CF_BF16"))],
                         ids=["sync-f16", "bf16x3"])
def test_cf_mfma_adversarial_routes(ops, orc, route, flags, name, T, D, window):
    """The same three signals on the cf32 kernels the default policy does not pick: the barrier-synchronous
    f16 kernel and the bf16 x 3 kernel (both have the direct path behind the zero-block / quiet-block test)."""
    x, taps, n_out, y64, bound = _cf_case(name, T, D, window)
    x_d, taps_d = _dev(x), _dev(taps)
    with _Policy(ops, flags):
        assert ops.fir_kernel_class(x_d, taps_d, D) == "cf-mfma"
        y = _host(ops.fir(taps_d, x_d, D, n_out))
        am = _host(ops.fir(taps_d, x_d, D, n_out, am=True))
    _check(y, y64, bound, (route, name, T, D))
    _check(am, np.abs(y64), bound, (route + "-am", name, T, D))


def test_cf_mfma_nonfinite_stays_local(ops, orc):
    """An inf / NaN sample reaches only the outputs whose window holds it, on the cf32 MFMA kernel."""
    T, D, n_out = 1023, 10, 20000
    n_in = (n_out - 1) * D + T
    x = orc.synth_wideband_cf32(7, 0.013, 0.31, 0, n_in)
    x[50_000] = np.inf
    x[120_003] = np.nan
    taps = orc.lowpass_taps(T, 0.04, "blackman")
    with _Policy(ops, ops.POLICY_NO_FFT):
        y = _host(ops.fir(_dev(taps), _dev(x), D, n_out))
    k = np.arange(n_out)
    touched = np.zeros(n_out, bool)
    for pos in (50_000, 120_003):
        touched |= (k * D <= pos) & (pos < k * D + T)
    leaked = np.nonzero(~np.isfinite(y) & ~touched)[0]
    assert leaked.size == 0, (int(leaked.size), leaked[:8].tolist(), (leaked[:8] // 512).tolist())
    y64, bound = orc.fir_f64(taps, x, D, n_out)
    _check(y[~touched], y64[~touched], bound[~touched], "nonfinite")


def _zero_gapped_iq(T, seed, n_sig=60_000):
    """int8 IQ: T + 500 zero samples, a signal, a zero gap of 2 T samples, the signal again, a short gap."""
    from oracle import synth_iq_int8
    sig = synth_iq_int8(0x5EED + seed, 1e9, 1e3, 7.5e7, 0, n_sig)
    half = 2 * (n_sig // 2)
    return np.concatenate([np.zeros(2 * (T + 500), np.int8), sig[:half], np.zeros(4 * T, np.int8), sig[half:],
                           np.zeros(2 * 37, np.int8)])


# The int8 routes: (policy flags, T, D, cutoff, window, kernel class). The first three keep the ids they had
# when the file ran the default policy only (the 4-way kernel is the default's choice with or without NO_FFT).
_C2 = [((), 127, 1, 0.1, "hamming", "i8-mfma")]
_W4 = [(("NO_FFT",), 1023, 10, 0.04, "blackman", "i8-dec-mfma"), (("NO_FFT",), 255, 5, 0.08, "blackman", "i8-dec-mfma")]
INT8_ROUTES = [pytest.param(*c, id="-".join(str(v) for v in c[1:])) for c in _W4 + _C2] + [
    pytest.param((), 127, 1, 0.1, "blackman", "i8-mfma", id="c2-127-blackman"),
    pytest.param((), 129, 1, 0.1, "blackman", "i8-mfma", id="c2-129-blackman"),  # S = 5 at the tap limit
    pytest.param((), 33, 1, 0.1, "blackman", "i8-mfma", id="c2-33-blackman"),    # S = 2
    pytest.param(("NO_FFT", "I8_WS8"), 1023, 10, 0.04, "blackman", "i8-dec-mfma", id="ws8-1023-10"),
    pytest.param(("NO_FFT", "I8_WS8"), 255, 5, 0.08, "blackman", "i8-dec-mfma", id="ws8-255-5"),
    pytest.param(("NO_FFT", "NO_WS"), 1023, 10, 0.04, "blackman", "i8-dec-mfma", id="sync-1023-10"),
    pytest.param(("NO_FFT", "NO_WS"), 255, 5, 0.08, "blackman", "i8-dec-mfma", id="sync-255-5"),
    # D = 16: no wave-specialised kernel takes a tile window of more than 8192 samples (31 D + T <= 1408)
    pytest.param((), 640, 16, 0.025, "blackman", "i8-dec-mfma", id="d16-640-16"),
]


@functools.lru_cache(maxsize=None)
def _int8_case(kind, T, D, cut, window):
    """An int8 stream, its taps and float64 reference, shared by the routes of one shape (read only)."""
    import oracle as orc
    iq = {"gapped": lambda: _zero_gapped_iq(T, T), "burst": lambda: _burst_onset_iq(120_000, 1, T),
          "zeros": lambda: np.zeros(2 * ((3 * 512 + 77) * D + T), np.int8)}[kind]()
    n_out = (len(iq) // 2 - T) // D + 1
    taps = orc.lowpass_taps(T, cut, window)
    y64, bound = orc.fir_f64(taps, orc.int8_to_float(iq).view(np.complex64), D, n_out)
    for a in (iq, taps, y64, bound):
        a.setflags(write=False)
    return iq, taps, n_out, y64, bound


def _run_int8(ops, flags, kind, T, D, cut, window, kernel):
    iq, taps, n_out, y64, bound = _int8_case(kind, T, D, cut, window)
    x_d, taps_d = _dev(iq), _dev(taps)
    with _Policy(ops, flags):
        assert ops.fir_kernel_class(x_d, taps_d, D, int8_iq=True) == kernel
        y = _host(ops.fir(taps_d, x_d, D, n_out, int8_iq=True))
        am = _host(ops.fir(taps_d, x_d, D, n_out, int8_iq=True, am=True))
    _check(y, y64, bound, ("int8-" + kind, kernel, flags, T, D))
    _check(am, np.abs(y64), bound, ("int8-" + kind + "-am", kernel, flags, T, D))
    return y, am


@pytest.mark.parametrize("flags,T,D,cut,window,kernel", INT8_ROUTES)
def test_int8_mfma_zero_padded_windows(ops, orc, flags, T, D, cut, window, kernel):
    """Every int8 MFMA route over a stream with a zero-padded start and exact-zero gaps: AM and complex
    outputs against float64 per element."""
    _run_int8(ops, flags, "gapped", T, D, cut, window, kernel)


def _burst_onset_iq(n, quiet, seed):
    """int8 IQ: +-quiet LSB of noise for the first half, then full-scale noise (a burst onset)."""
    rng = np.random.default_rng(seed)
    q = np.where(np.arange(2 * n) < n, rng.integers(-quiet, quiet + 1, 2 * n), rng.integers(-128, 128, 2 * n))
    return q.astype(np.int8)


@pytest.mark.parametrize("flags,T,D,cut,window,kernel", INT8_ROUTES)
def test_int8_mfma_burst_onset(ops, orc, flags, T, D, cut, window, kernel):
    """VERDICT r05 item 3's int8 x int8 form fails here (tools/exp/q8_tap_error.py --burst: 1.7-2.4x the
    bound): the windows with a full-scale burst under the tail taps and +-1 LSB under the large ones. The
    product's f16 x 2 tap limbs keep each tap to 2^-22 of itself: per element within the bound."""
    _run_int8(ops, flags, "burst", T, D, cut, window, kernel)


@pytest.mark.parametrize("flags,T,D,cut,window,kernel", INT8_ROUTES)
def test_int8_mfma_all_zero_stream(ops, orc, flags, T, D, cut, window, kernel):
    """An all-zero stream (a few tiles, the last partial): every output is exactly 0 - the bound is 0 - and the
    guard, which skips windows that are zero throughout, leaves that to the MFMA path."""
    y, am = _run_int8(ops, flags, "zeros", T, D, cut, window, kernel)
    assert not y.any() and not am.any()


def _many_gaps_iq(n_in, period, gap, seed):
    """Full-scale int8 IQ noise with an exact-zero gap of `gap` samples every `period` samples - the period is
    odd and no multiple of a tile's input span, so the zero / signal edges walk through every alignment and
    every tile of a block's range - a zero-padded start, and one stretch of four periods zero throughout."""
    rng = np.random.default_rng(seed)
    iq = rng.integers(-128, 128, 2 * n_in).astype(np.int8).reshape(n_in, 2)
    iq[np.arange(n_in) % period < gap] = 0
    iq[n_in // 2: n_in // 2 + 4 * period] = 0
    return iq.reshape(-1)


# The guards' per-tile state in a block's LATER tiles. A launch of at most 768 (C2) or 256 (decimating) tiles
# gives every block one tile: chunk 0, wave 0, parity 0 - all the cases above. Here each block owns several:
#   C2           7680 tiles on 768 blocks: 10 each, chunk 0 (waves 0-3, both tiles of a wave) and chunk 1 - the
#                flag words of every wave and tile slot, both chunk parities and the re-zeroing between them;
#   synchronous  768 tiles on 256 blocks: 3 each (block-local tiles 1 and 2: both parities of the hand-over);
#   D = 16       520 tiles: 2-3 each on the G = 3 instantiation that only the shape routes to.
# Gaps of ~2 T every ~3.3 (C2) / ~1.4 / ~0.6 tiles put flagged tiles at every position. On the limb emulation
# (tests/mfma_inputs.py) each stream has outputs outside the bound in tiles at every such position: about one
# per 600 to 850 outputs in the first 150 000.
LATER_TILES = [pytest.param((), 127, 1, 0.1, "i8-mfma", 7680, 1671, 254, id="c2-10-tiles-per-block"),
               pytest.param(("NO_FFT", "NO_WS"), 255, 5, 0.08, "i8-dec-mfma", 768, 3511, 510, id="sync-3-tiles-per-block"),
               pytest.param((), 640, 16, 0.025, "i8-dec-mfma", 520, 5003, 1280, id="d16-3-tiles-per-block")]


@pytest.mark.parametrize("flags,T,D,cut,kernel,tiles,period,gap", LATER_TILES)
def test_int8_mfma_gaps_in_later_tiles(ops, orc, flags, T, D, cut, kernel, tiles, period, gap):
    """Blackman filters over a stream of many exact-zero gaps, in launches where every block walks several
    tiles (and, on C2, two chunks): complex and AM outputs against float64 per element, the last tile partial."""
    n_out = tiles * 512 - 77
    iq = _many_gaps_iq((n_out - 1) * D + T, period, gap, T)
    taps = orc.lowpass_taps(T, cut, "blackman")
    x_d, taps_d = _dev(iq), _dev(taps)
    with _Policy(ops, flags):
        assert ops.fir_kernel_class(x_d, taps_d, D, int8_iq=True) == kernel
        y = _host(ops.fir(taps_d, x_d, D, n_out, int8_iq=True))
        am = _host(ops.fir(taps_d, x_d, D, n_out, int8_iq=True, am=True))
    y64, bound = orc.fir_f64(taps, orc.int8_to_float(iq).view(np.complex64), D, n_out)
    _check(y, y64, bound, ("int8-later-tiles", kernel, flags, T, D))
    _check(am, np.abs(y64), bound, ("int8-later-tiles-am", kernel, flags, T, D))


def _comb_routes():
    c2 = [pytest.param((), "i8-mfma", *c, id=f"c2-{c[3]}") for c in mi.COMB_C2]
    dec = [pytest.param(flags, "i8-dec-mfma", *c, id=f"{name}-{c[0]}-{c[1]}")
           for name, flags in (("ws4", ("NO_FFT",)), ("ws8", ("NO_FFT", "I8_WS8")), ("sync", ("NO_FFT", "NO_WS")))
           for c in mi.COMB_DEC]
    return c2 + dec


@functools.lru_cache(maxsize=None)
def _comb_case(T, D, cut, window, n_out, k0s):
    import oracle as orc
    iq = mi.comb_iq(T, D, cut, n_out, k0s)
    taps = orc.lowpass_taps(T, cut, window)
    xc = orc.int8_to_float(iq).view(np.complex64)
    y64, bound = orc.fir_f64(taps, xc, D, n_out)
    floor = mi.LIMB_FLOOR * float(np.max(np.abs(taps))) * mi.window_abs_sum(xc, T, D, n_out)
    for a in (iq, taps, y64, bound, floor):
        a.setflags(write=False)
    return iq, taps, y64, bound, floor


@pytest.mark.parametrize("flags,kernel,T,D,cut,window,n_out,k0s", _comb_routes())
def test_int8_mfma_comb_under_sinc_zeros(ops, orc, flags, kernel, T, D, cut, window, n_out, k0s):
    """The hole the zero-window guard leaves: int8 IQ with no zero sample except in the windows
    of a few engineered outputs, where only the samples under the windowed sinc's zeros (taps ~1e-17 of the
    peak, gone from both f16 limbs) stay non-zero. No zero run exceeds 15 samples, so no tile is flagged and the
    MFMA path runs. Asserted: every other output meets 1e-6 sum|h||x|; every output, engineered ones included,
    meets 1e-6 sum|h||x| + 2^-39 max|h| sum|x| - the limbs' floor, derived in tests/mfma_inputs.py and pinned on
    the CPU in tests/test_mfma_limbs.py; and the VALU form (GSDR_POLICY_NO_MFMA) meets the plain bound
    everywhere on the same input. Whether the MFMA kernels miss the plain bound at the engineered outputs is
    printed, not asserted (a later guard may close the hole); DESIGN.md 9 records the measured ratios."""
    iq, taps, y64, bound, floor = _comb_case(T, D, cut, window, n_out, k0s)
    assert mi.longest_zero_run(iq) <= 15
    x_d, taps_d = _dev(iq), _dev(taps)
    with _Policy(ops, flags):
        assert ops.fir_kernel_class(x_d, taps_d, D, int8_iq=True) == kernel
        y = _host(ops.fir(taps_d, x_d, D, n_out, int8_iq=True))
        am = _host(ops.fir(taps_d, x_d, D, n_out, int8_iq=True, am=True))
    with _Policy(ops, ("NO_MFMA", "NO_FFT")):  # the VALU direct form
        valu = ops.fir_kernel_class(x_d, taps_d, D, int8_iq=True)
        assert "mfma" not in valu and "fft" not in valu, valu
        yv = _host(ops.fir(taps_d, x_d, D, n_out, int8_iq=True))
        amv = _host(ops.fir(taps_d, x_d, D, n_out, int8_iq=True, am=True))
    eng = np.zeros(n_out, bool)
    eng[list(k0s)] = True
    for got, want, what in ((y, y64, "complex"), (am, np.abs(y64), "am")):
        err = np.abs(got.astype(np.complex128) - want)
        print(f"comb {kernel} {flags} T={T} D={D} {window} {what}: worst err / (1e-6 bound) engineered "
              f"{float(np.max(err[eng] / (FIR_TOL * bound[eng]))):.3g}, elsewhere "
              f"{float(np.max(err[~eng] / (FIR_TOL * bound[~eng]))):.3g}; worst err / (1e-6 bound + floor) "
              f"{float(np.max(err / (FIR_TOL * bound + floor))):.3g}")
        _check(got[~eng], want[~eng], bound[~eng], ("comb-elsewhere", what, kernel, flags, T, D))
        over = np.nonzero(~(err <= FIR_TOL * bound + floor))[0]
        assert over.size == 0, (what, kernel, flags, [(int(k), float(err[k] / (FIR_TOL * bound[k] + floor[k])))
                                                      for k in over[:8]])
    _check(yv, y64, bound, ("comb-valu", T, D))
    _check(amv, np.abs(y64), bound, ("comb-valu-am", T, D))


@pytest.mark.parametrize("flags", [(), ("I8_WS8",)], ids=["ws4", "ws8"])
def test_fused_chain_zero_padded_windows(ops, orc, flags):
    """The fused C5 chain (RF FIR -> AM -> audio FIR in one launch) over the zero-gapped stream, on the 4-way
    kernel and on the 8-way one (GSDR_POLICY_I8_WS8): the AM samples against float64 per element, the audio
    within the carried bound."""
    import torch
    T, D, Ta, Da = 1023, 10, 255, 20
    iq = _zero_gapped_iq(T, 3, n_sig=400_000)
    n_in = len(iq) // 2
    n_rf = (n_in - T) // D + 1
    n_audio = (n_rf - Ta) // Da + 1
    rf, au = orc.lowpass_taps(T, 0.04, "blackman"), orc.lowpass_taps(Ta, 0.02)
    am = torch.zeros(n_rf, dtype=torch.float32, device="cuda")
    audio = torch.empty(n_audio, dtype=torch.float32, device="cuda")
    with _Policy(ops, flags):
        ops.am_chain_fused(_dev(rf), _dev(iq), D, n_rf, am, 0, _dev(au), Da, n_audio, audio, store_am=True)
    xc = orc.int8_to_float(iq).view(np.complex64)
    y64, rf_bound = orc.fir_f64(rf, xc, D, n_rf)
    _check(_host(am), np.abs(y64), rf_bound, "fused-am")
    a64 = np.abs(y64)
    want, audio_bound = orc.fir_f64(au, a64.astype(np.float32), Da, n_audio)
    carried, _ = orc.fir_f64(np.abs(au), (FIR_TOL * (rf_bound + a64)).astype(np.float32), Da, n_audio)
    got = _host(audio)
    bad = np.nonzero(~(np.abs(got - want) <= carried + FIR_TOL * audio_bound + 1e-30))[0]
    assert bad.size == 0, (int(bad.size), bad[:8].tolist())
