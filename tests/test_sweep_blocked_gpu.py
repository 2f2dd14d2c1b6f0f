"""A 54- / 30-layer longwave gas holds the operands of its mirror sweep line-blocked (csrc/sweep_layout.hpp: the Planck
matrix and the background as [n / 16][rows][16]) and is swept by k_rt_lw_bb_mirror<.., .., true> (csrc/find_g.hip); a gas
made with ECCKD_RT_ROWMAJOR=1 keeps the row-major matrices and the row-major kernel.  Only the addresses of the loads
differ, so nothing here has a tolerance:

  a. the errors of both gases have the same bits: spectra of 16 * 37 and of 2 048 points, intervals whose first index is 0, 1
     and 15 modulo 16, of 1, 15, 16, 17, 63, 64, 65, 127, 128, 129 and 257 points and the whole band, each alone, all in one
     batch, and the band cut into 1, 2 and 7 intervals; 54 layers with a DOUBLE background (DOUBLE rows) and with a FLOAT
     one (FLOAT pairs and the shared middle pair), 30 layers (15 per half: the single last layer and, with pairs, its load);
  b. the bg_optical_depth and planck_hl views of the blocked gas - the first rebuilt from the blocked matrix - equal the
     row-major gas's, and the blocked Planck matrix is the row-major one in the layout of the header;
  c. a gas given the first gas's planck_hl shares its blocked copy, a gas given the same matrix in a buffer nobody knows
     makes its own: same errors; and the same again from the shared copy after the first gas is destroyed;
  d. a spectrum of 601 points has rows that are no whole lines: no blocked copy, the same errors with and without the knob;
  e. a whole search over 4 096 points returns the same bounds, status and errors under both settings."""
import numpy as np
import pytest

from test_find_g_gpu import _dev
from test_interval_edges_gpu import FLUX_WEIGHT
from test_sweep_alignment_gpu import METHOD, _problem

pytestmark = pytest.mark.gpu

LENGTHS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)
CASES = [(592, 54, "double"), (592, 54, "float"), (2048, 54, "double"), (2048, 54, "float"), (592, 30, "double"), (592, 30, "float")]


@pytest.fixture(autouse=True)
def _every_request_on_the_device(monkeypatch):
    monkeypatch.setenv("ECCKD_NO_ERROR_MEMO", "1")
    for knob in ("ECCKD_RT_ROWMAJOR", "ECCKD_RT_UNALIGNED", "ECCKD_RT_GENERIC", "ECCKD_BG64"):
        monkeypatch.delenv(knob, raising=False)


def intervals(n):
    """[(i1, i2)] inclusive: every length from every residue of the first index, then the whole band."""
    iv = [(32 + 16 * k + r, 32 + 16 * k + r + m - 1) for k, m in enumerate(LENGTHS) for r in (0, 1, 15)]
    iv.append((0, n - 1))
    assert all(0 <= a <= b < n for a, b in iv) and {a % 16 for a, _ in iv} == {0, 1, 15}
    return iv


def _gas(ctx, o, nlay, bg_kind, **kw):
    from ecckd_amd import api
    gas = api.GasLW(ctx, o["p"], o["t_hl"], _dev(ctx, o["wn"]), _dev(ctx, o["dwn"]), _dev(ctx, o["rank"].astype(np.int32)),
                    _dev(ctx, o["od"].astype(np.float32 if nlay == 54 else np.float64)), _dev(ctx, o["bg"]), METHOD, FLUX_WEIGHT, **kw)
    # FLOAT pairs or DOUBLE rows, whichever layout holds them
    assert gas.sweep_bytes_per_point() == (nlay + 1) * 8 + nlay * (4 if bg_kind == "float" else 8)
    return gas


def _is_blocked(gas):
    from ecckd_amd.api import EcckdError
    try:
        return gas.view_ptr("planck_hl_blocked")[0] is not None
    except EcckdError:
        return False


def _pair(ctx, monkeypatch, o, nlay, bg_kind):
    """(blocked gas, row-major gas) from the same inputs; the knob belongs to the gas."""
    blocked = _gas(ctx, o, nlay, bg_kind)
    monkeypatch.setenv("ECCKD_RT_ROWMAJOR", "1")
    rowmajor = _gas(ctx, o, nlay, bg_kind)
    monkeypatch.delenv("ECCKD_RT_ROWMAJOR")
    return blocked, rowmajor


def _all_forms(gas, n):
    """The errors in every batch form of a., one array."""
    iv = intervals(n)
    out = [np.array([gas.calc_error_batch(a, b - a + 1, [0.0], [1.0])[0] for a, b in iv]),
           gas.calc_error_multi(np.array([a for a, _ in iv]), np.array([b - a + 1 for a, b in iv]), np.zeros(len(iv)), np.ones(len(iv)))]
    for parts in (1, 2, 7):
        cuts = np.linspace(0.0, 1.0, parts + 1)
        out.append(gas.calc_error_batch(0, n, cuts[:-1], cuts[1:]))
    return np.concatenate(out)


@pytest.mark.parametrize("n,nlay,bg_kind", CASES)
def test_same_errors_bit_for_bit(ctx, oracle, monkeypatch, n, nlay, bg_kind):
    """a. and b."""
    assert n % 16 == 0
    o = _problem(oracle, n, nlay, bg_kind)
    blocked, rowmajor = _pair(ctx, monkeypatch, o, nlay, bg_kind)
    assert _is_blocked(blocked) and not _is_blocked(rowmajor)
    got, want = _all_forms(blocked, n), _all_forms(rowmajor, n)
    assert np.all(np.isfinite(want)) and np.all(want >= 0.0) and np.count_nonzero(want) > want.size // 2
    assert np.array_equal(got, want)
    # alone and in one batch: one layout of chunks either way (chunk_layout.hpp)
    m = len(intervals(n))
    assert np.array_equal(got[:m], got[m:2 * m])

    # b. the views; the blocked matrix is [n / 16][nlay + 1][16]
    planck = rowmajor.view("planck_hl")
    assert np.array_equal(blocked.view("planck_hl"), planck)
    assert np.array_equal(blocked.view("bg_optical_depth"), rowmajor.view("bg_optical_depth"))
    assert np.array_equal(blocked.view("bg_optical_depth"), o["bg_s"])
    raw = blocked.view("planck_hl_blocked")
    assert np.array_equal(raw.reshape(n // 16, nlay + 1, 16).transpose(1, 0, 2).reshape(nlay + 1, n), planck)
    # ... and the run-time-nlay sweep of the blocked gas still finds its rows
    monkeypatch.setenv("ECCKD_RT_GENERIC", "1")
    cuts = np.linspace(0.0, 1.0, 4)
    generic = blocked.calc_error_batch(0, n, cuts[:-1], cuts[1:])
    assert np.array_equal(generic, rowmajor.calc_error_batch(0, n, cuts[:-1], cuts[1:])) and np.all(generic > 0.0)
    monkeypatch.delenv("ECCKD_RT_GENERIC")
    assert np.array_equal(_all_forms(blocked, n), want)          # after the rows were rebuilt for the view
    blocked.close()
    rowmajor.close()


@pytest.mark.parametrize("bg_kind", ["double", "float"])
def test_gases_that_share_a_planck_matrix_share_its_blocked_copy(ctx, oracle, bg_kind):
    """c."""
    n, nlay = 592, 54
    o = _problem(oracle, n, nlay, bg_kind)
    first = _gas(ctx, o, nlay, bg_kind)
    want = _all_forms(first, n)
    second = _gas(ctx, o, nlay, bg_kind, planck_hl_reuse=first.view_ptr("planck_hl")[0])
    stranger = _dev(ctx, first.view("planck_hl"))           # the same matrix where the context's table has no entry
    assert stranger.data_ptr() % 128 == 0
    third = _gas(ctx, o, nlay, bg_kind, planck_hl_reuse=stranger.data_ptr())
    shared = first.view_ptr("planck_hl_blocked")[0]
    assert second.view_ptr("planck_hl_blocked")[0] == shared and third.view_ptr("planck_hl_blocked")[0] != shared
    assert np.array_equal(third.view("planck_hl_blocked"), first.view("planck_hl_blocked"))
    assert np.array_equal(_all_forms(second, n), want)
    assert np.array_equal(_all_forms(third, n), want)
    first.close()                                           # the copy lives on with its second holder
    assert second.view_ptr("planck_hl_blocked")[0] == shared
    assert np.array_equal(_all_forms(second, n), want)
    assert np.array_equal(_all_forms(third, n), want)
    second.close()
    third.close()
    del stranger


@pytest.mark.parametrize("nlay,bg_kind", [(54, "double"), (54, "float")])
def test_rows_that_are_no_whole_lines_stay_row_major(ctx, oracle, monkeypatch, nlay, bg_kind):
    """d."""
    n = 601
    o = _problem(oracle, n, nlay, bg_kind)
    default, knob = _pair(ctx, monkeypatch, o, nlay, bg_kind)
    assert not _is_blocked(default) and not _is_blocked(knob)
    iv = [(a, b) for a, b in intervals(592)] + [(0, n - 1), (n - 1, n - 1)]
    starts, lens = np.array([a for a, _ in iv]), np.array([b - a + 1 for a, b in iv])
    got = default.calc_error_multi(starts, lens, np.zeros(len(iv)), np.ones(len(iv)))
    want = knob.calc_error_multi(starts, lens, np.zeros(len(iv)), np.ones(len(iv)))
    assert np.all(np.isfinite(want)) and want[-2] > 0.0
    assert np.array_equal(got, want)
    default.close()
    knob.close()


def test_whole_search_is_the_same(ctx, oracle, monkeypatch):
    """e."""
    n, nlay = 4096, 54
    o = _problem(oracle, n, nlay, "double")
    monkeypatch.delenv("ECCKD_NO_ERROR_MEMO")               # the search as it runs
    blocked, rowmajor = _pair(ctx, monkeypatch, o, nlay, "double")
    assert _is_blocked(blocked) and not _is_blocked(rowmajor)
    st_b, bounds_b, err_b, cost_b = blocked.find_g_band(0, n - 1, 0.05, 0.02, 40)
    st_r, bounds_r, err_r, cost_r = rowmajor.find_g_band(0, n - 1, 0.05, 0.02, 40)
    assert len(err_r) >= 2 and np.all(np.isfinite(err_r))
    assert st_b == st_r and cost_b == cost_r
    assert np.array_equal(bounds_b, bounds_r) and np.array_equal(err_b, err_r)
    blocked.close()
    rowmajor.close()
