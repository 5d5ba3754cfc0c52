"""tests/_transform_reference.py, the long-double restatement that tests/test_gpu_transforms.py compares the range, Doppler and OFDM kernels with, checked
without a GPU:
  * against the project's fp64 oracle (O.rdm_explicit, O.ofdm_modulate, O.ofdm_demodulate) at every shape the GPU file runs, within 1e-12 rms, and against
    O.fft2d's own map on one physical scene;
  * its comparison rule ``check`` rejects five small, realistic errors;
  * the two cyclic-prefix terms are whole numbers for Nfft = 128..4096 at every numerology and are not at Nfft = 64 (why the library refuses that carrier)."""
from __future__ import annotations

import numpy as np
import pytest

import _transform_reference as R
import oracle as O
from conftest import make_scene

RTOL = 1e-12          # oracle against reference, relative to the reference's rms


def _close(oracle64, ref):
    m = R.measure(oracle64, ref, oracle64)
    assert m.e_ref <= RTOL * m.rms, f"oracle vs reference: {m.e_ref / m.rms:.3e} rms at {m.idx}"
    return m


# ------------------------------------------------------------------ the restatement against the oracle
@pytest.mark.parametrize("c", R.PLANE_CASES, ids=R.case_id)
def test_plane_reference_matches_oracle(c):
    rx, tx = R.plane_inputs(c)
    rows, a = R.plane_rows(c), c["ant"]
    ref = R.rdm_plane(rx[:, :, a], tx[:, :, a], c["n_ifft"], c["n_fft"], rows)
    m = _close(O.rdm_explicit(rx, tx, c["n_ifft"], c["n_fft"])[rows, :, a], ref)
    assert m.peak < 8 * m.rms                              # noise-like: every cell has a comparable magnitude


@pytest.mark.parametrize("c", R.WINDOW_CASES, ids=R.case_id)
def test_window_reference_matches_oracle(c):
    rx, tx, amp, added = R.window_inputs(c)
    r_lo, nr, c_lo, nc = R.window_geometry(c)
    assert r_lo >= 0 and r_lo + nr <= c["n_ifft"] and c_lo >= 0 and c_lo + nc <= c["n_fft"]
    assert (c["n_fft"] + min(c["L"], c["n_fft"]) * 17) * 16 <= 160 * 1024      # the Doppler kernels' LDS
    assert added < 0.10                                    # the tone adds less than 10 % to the grid's energy
    rows = np.arange(r_lo, r_lo + nr)
    full = O.rdm_explicit(rx, tx, c["n_ifft"], c["n_fft"])
    for a in (0, c["A"] - 1):
        ref = np.abs(R.rdm_plane(rx[:, :, a], tx[:, :, a], c["n_ifft"], c["n_fft"], rows)[:, c_lo:c_lo + nc]) ** 2
        _close(np.abs(full[r_lo:r_lo + nr, c_lo:c_lo + nc, a]) ** 2, ref)
        # the tone's cell is a CUT, about 50 times over the floor: the floor at its row is sum w_k^2 Lu w_r[row]^2 / (nIFFT nFFT) for unit-variance noise
        tr, tc = c["r0"], (c["d0"] + c["n_fft"] // 2) % c["n_fft"]
        assert c["rows"][0] <= tr + 1 <= c["rows"][1] and c["cols"][0] <= tc + 1 <= c["cols"][1]
        wk, wr = R.kaiser(c["K"], 3), R.kaiser(c["n_ifft"], 3)[R.fftshift_index(c["n_ifft"])]
        floor = float((wk * wk).sum() * min(c["L"], c["n_fft"]) * wr[tr] ** 2) / (c["n_ifft"] * c["n_fft"])
        assert 20 < float(ref[tr - r_lo, tc - c_lo]) / floor < 100


@pytest.mark.parametrize("c", R.OFDM_CASES, ids=R.case_id)
def test_ofdm_reference_matches_oracle(c):
    grid, wave = R.ofdm_inputs(c)
    td_idx, rows = R.ofdm_subsets(c)
    ref = R.ofdm_modulate(grid, c["nfft"], c["scs"], td_idx=td_idx)
    keep = np.isfinite(ref.real)
    assert keep.sum() >= min(ref.size, 90 * c["L"] * c["A"])
    m = _close(O.ofdm_modulate(grid, c["nfft"], c["scs"])[keep], ref[keep])
    assert m.peak < 8 * m.rms
    ref = R.ofdm_demodulate(wave, c["n_sc"], c["nfft"], c["scs"], rows)
    assert ref.shape[1] == c["L"]
    want = O.ofdm_demodulate(wave, c["n_sc"], c["nfft"], c["scs"])
    m = _close(want if rows is None else want[rows], ref)
    assert m.peak < 8 * m.rms


@pytest.mark.parametrize("c", R.WINDOWED_CASES, ids=R.case_id)
def test_windowed_modulator_reference_matches_oracle(c):
    first = (c["n_slot"] % (c["scs"] // 15)) * 14
    grid, _ = R.ofdm_inputs(c, first_symbol=first)
    ref = R.ofdm_modulate(grid, c["nfft"], c["scs"], c["windowing"], first)
    _close(O.ofdm_modulate(grid, c["nfft"], c["scs"], c["windowing"], first), ref)
    assert np.abs(ref - R.ofdm_modulate(grid, c["nfft"], c["scs"], 0, first)).max() > 1e-3      # the windowing does something


def test_reference_matches_fft2d_on_a_physical_scene():
    """One small cell through the oracle's chain: the restatement equals the map fft2D.m:37-46 gives literally (O.rdm_literal inside O.fft2d)."""
    sc = make_scene(n_ants=4, n_slots=4, nrb=24, targets=((150.0, 40.0, 1.5),), velocity=(0.0,), num_slots_param=6, zero_s_slots=False)   # smoke()'s cell
    echo = O.mono_static_sensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, sc.rp, sc.los, sc.noise, nfft=sc.wave.Nfft)
    est, dbg = O.fft2d(sc.rp, O.cfar2d_config(sc.rp), echo, sc.tx_grid, return_debug=True)
    assert est.rngEst.size >= 1
    for a in (0, sc.A - 1):
        ref = R.rdm_plane(echo[:, :, a], sc.tx_grid[:, :, a], int(sc.rp.nIFFT), int(sc.rp.nFFT))
        # (a target's peak stands far over the map's rms here: the oracle's rounding scales with the peak)
        assert np.abs(dbg.rdm[:, :, a] - ref).max() <= RTOL * float(np.abs(ref).max())


# ------------------------------------------------------------------ the comparison rule is sensitive
@pytest.fixture(scope="module")
def odd_plane():
    c = R.PLANE_CASES[3]                                   # K 200, nIFFT 256, L 13 (odd), nFFT 32
    rx, tx = R.plane_inputs(c)
    ref = R.rdm_plane(rx[:, :, 0], tx[:, :, 0], c["n_ifft"], c["n_fft"])
    o64 = O.rdm_explicit(rx, tx, c["n_ifft"], c["n_fft"])[:, :, 0]
    return c, rx, tx, ref, o64


def test_check_accepts_the_oracle_and_returns_the_worst_index(odd_plane):
    c, rx, tx, ref, o64 = odd_plane
    seen = []
    idx = R.check(o64, ref, o64, report=seen.append)
    assert len(idx) == 2 and seen[0].idx == idx and seen[0].err == seen[0].e_ref
    assert 1e-16 < seen[0].e_ref / seen[0].rms < 1e-14


def _rejected(got, ref, o64):
    with pytest.raises(AssertionError, match="worst element"):
        R.check(got, ref, o64)


def test_check_rejects_two_adjacent_rows_swapped(odd_plane):
    _, _, _, ref, o64 = odd_plane
    got = o64.copy()
    got[[100, 101]] = got[[101, 100]]
    _rejected(got, ref, o64)


def test_check_rejects_one_doppler_column_rolled(odd_plane):
    _, _, _, ref, o64 = odd_plane
    got = o64.copy()
    got[:, 7] = np.roll(got[:, 7], 1)
    _rejected(got, ref, o64)


def test_check_rejects_one_cell_moved_by_1e_12_rms(odd_plane):
    _, _, _, ref, o64 = odd_plane
    got = o64.copy()
    got[17, 5] += 1e-12 * float(np.sqrt(np.mean(np.abs(ref) ** 2)))
    _rejected(got, ref, o64)


def test_check_rejects_the_wrong_ifftshift_half_at_odd_l(odd_plane):
    c, rx, tx, ref, o64 = odd_plane
    assert c["L"] % 2 == 1
    got = R.rdm_plane(rx[:, :, 0], tx[:, :, 0], c["n_ifft"], c["n_fft"], l_shift=(c["L"] + 1) // 2).astype(np.complex128)
    _rejected(got, ref, o64)
    same = R.rdm_plane(rx[:, :, 0], tx[:, :, 0], c["n_ifft"], c["n_fft"], l_shift=c["L"] // 2).astype(np.complex128)
    R.check(same, ref, o64)


def test_check_rejects_the_cp_offset_rounded_up_at_an_odd_cp():
    c = R.OFDM_CASES[0]                                    # Nfft 128 at 15 kHz: CPs of 9 and 10 samples
    assert set(R.cp_lengths(c["nfft"], c["scs"], c["L"])) == {9, 10}
    _, wave = R.ofdm_inputs(c)
    ref = R.ofdm_demodulate(wave, c["n_sc"], c["nfft"], c["scs"])
    o64 = O.ofdm_demodulate(wave, c["n_sc"], c["nfft"], c["scs"])
    R.check(o64, ref, o64)
    got = R.ofdm_demodulate(wave, c["n_sc"], c["nfft"], c["scs"], cp_offset=lambda cp: (cp + 1) // 2).astype(np.complex128)
    assert np.array_equal(got[:, 0], ref[:, 0].astype(np.complex128))          # l = 0: CP 10, fix == ceil
    _rejected(got, ref, o64)


# ------------------------------------------------------------------ cyclic-prefix lengths
def test_cp_terms_are_whole_from_128_points_and_not_at_64():
    for mu, scs in enumerate((15, 30, 60, 120)):
        for nfft in (128, 256, 512, 1024, 2048, 4096):
            base, extra, m = R.cp_terms(nfft, scs)
            assert m == mu and base.denominator == 1 and extra.denominator == 1
            n = 28 * 2 ** mu + 3
            for first in (0, 14):
                assert np.array_equal(R.cp_lengths(nfft, scs, n, first), O.cp_lengths(nfft, scs, n, first))
        base, extra, _ = R.cp_terms(64, scs)
        assert base.denominator == 2                        # 144 * 64 / 2048 = 4.5: no normal CP of whole samples below nrOFDMInfo's minimum Nfft
        assert (extra.denominator == 2) == (mu == 0)
        with pytest.raises(AssertionError, match="no integral cyclic prefix"):
            R.cp_lengths(64, scs, 14)
