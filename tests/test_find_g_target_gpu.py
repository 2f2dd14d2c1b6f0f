"""ecckd_find_g_gases_target: the searches of several prepared gases at the tolerance scaling that gives a wanted total number
of g points.  A trial is ecckd_find_g_gases as it stands on the gases as prepared, with their memos of interval errors kept
from trial to trial, so the answer must be - bit for bit - what a plain run at the reported tolerances gives, with or without
the memo."""
import numpy as np
import pytest
import torch

from conftest import make_lw_case

pytestmark = pytest.mark.gpu

NWAV, NGAS = 60000, 4
TOLTOL, ITER = 0.02, 30
RESOLUTION = 1e-3


def _dev(ctx, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=ctx.device)


def _gases(ctx, nwav, nlay, ngas, double_bg):
    """As tests/test_find_g_gases_gpu.py::_gases; also hands back the wavenumbers and ranks (for the refusal of a base split)."""
    from ecckd_amd import api, synthetic as syn
    out, extra = [], []
    first = None
    for k in range(ngas):
        p, wn, dwn, od = make_lw_case(nwav, nlay, seed=31 + k, nlines=40 + 7 * k, column_scale=[30.0, 100.0, 5.0, 50.0][k % 4])
        _, _, _, bg = make_lw_case(nwav, nlay, seed=131 + k, nlines=24, column_scale=3.0)
        if double_bg:
            bg = bg.astype(np.float64) * 0.4337 + make_lw_case(nwav, nlay, seed=231 + k, nlines=12, column_scale=1.0)[3].astype(np.float64)
        t = syn.temperature_profile(p)
        d_wn = _dev(ctx, wn)
        key, _ = api.reorder_key_lw(ctx, p, api.idealised_temperature(p), d_wn, _dev(ctx, dwn), _dev(ctx, od), 0.5)
        rnk, _ = api.stable_argsort_bands(ctx, key, [0], [nwav - 1], want_ordered=False)
        gas = api.GasLW(ctx, p, t, d_wn, _dev(ctx, dwn), rnk, _dev(ctx, od), _dev(ctx, bg), "transmission", 0.0,
                        planck_hl_reuse=first.view_ptr("planck_hl")[0] if first is not None else None)
        first = first or gas
        out.append(gas)
        extra.append((d_wn, rnk))
    return out, extra


_CACHE = {}


@pytest.fixture(scope="module")
def prepared(ctx):
    """The four gases at 54 and at 20 layers, prepared once for the module: get(nlay) -> (gases, [(wavenumber, rank)])."""
    def get(nlay):
        if nlay not in _CACHE:
            _CACHE[nlay] = _gases(ctx, NWAV, nlay, NGAS, True)
        return _CACHE[nlay]
    yield get
    for gases, _ in _CACHE.values():
        for g in gases:
            g.close()
    _CACHE.clear()


def _reset(gases):
    for g in gases:
        g.reset_memo()


def _req(tol, edges=(0, NWAV), options=None):
    edges = list(edges)
    nband = len(edges) - 1
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), (nband,))
    return dict(ibegin=edges[:-1], iend=[e - 1 for e in edges[1:]], heating_rate_tolerance=tol.copy(), options=options)


def _total(res, ng_offset):
    return ng_offset + sum(len(r["error"]) for g_res in res for r in g_res)


def _same(a, b):
    """Two results of find_g_gases, per gas and band: the same decisions to the last bit."""
    assert len(a) == len(b)
    for ga, gb in zip(a, b):
        assert len(ga) == len(gb)
        for ra, rb in zip(ga, gb):
            assert ra["status"] == rb["status"]
            assert np.array_equal(ra["rank1"], rb["rank1"]) and np.array_equal(ra["rank2"], rb["rank2"])
            assert ra["bounds"].tobytes() == rb["bounds"].tobytes() and ra["error"].tobytes() == rb["error"].tobytes()


def _straddled(info, target, resolution):
    """Two trials either side of the target whose scalings are within 1 + resolution of each other."""
    above = [s for s, n in info["trials"] if n > target]
    below = [s for s, n in info["trials"] if n < target]
    return any(lo < hi and hi / lo <= 1.0 + resolution for lo in above for hi in below)


_OUTCOMES = {}


def _reproduce(gases, nlay):
    """For N0 (what a plain run at tolerance 0.05 gives), N0 + 3 and N0 - 2: search the target from the first guess 0.2 and
    compare with plain runs at the reported tolerances.  -> [(target, info)]; computed once per nlay."""
    from ecckd_amd import api
    if nlay in _OUTCOMES:
        return _OUTCOMES[nlay]
    ng_offset = 1 - NGAS
    _reset(gases)
    n0 = _total(api.find_g_gases(gases, [_req(0.05) for _ in gases], TOLTOL, ITER), ng_offset)
    assert n0 >= NGAS + 4
    out = []
    for target in (n0, n0 + 3, n0 - 2):
        _reset(gases)
        res, info = api.find_g_gases_target(gases, [_req(0.2) for _ in gases], ng_offset, target, RESOLUTION, 40, TOLTOL, ITER)
        print(f"nlay {nlay} target {target}: status {info['status']} ng {info['ng']} scaling {info['scaling']!r} "
              f"trials {info['trials']}")
        assert _total(res, ng_offset) == info["ng"]
        assert (info["scaling"], info["ng"]) in info["trials"]
        used = info["tolerance_used"]
        assert all(u.shape == (1,) and u[0] == info["scaling"] * 0.2 for u in used)
        # a plain run at those tolerances, memo reset: the same bits; and again, now answered from the memo
        _reset(gases)
        plain = api.find_g_gases(gases, [_req(u) for u in used], TOLTOL, ITER)
        _same(res, plain)
        _same(res, api.find_g_gases(gases, [_req(u) for u in used], TOLTOL, ITER))
        if info["ng"] == target:
            assert info["status"] == 0
        else:
            # accepted only where the count steps over the target within the resolution
            assert info["status"] == 1 and _straddled(info, target, RESOLUTION), info
        out.append((target, info))
    _OUTCOMES[nlay] = out
    return out


@pytest.mark.parametrize("nlay", [54, 20])
def test_reproduces_a_plain_run(prepared, nlay):
    gases, _ = prepared(nlay)
    assert len(_reproduce(gases, nlay)) == 3


def test_at_least_four_of_six_targets_are_hit_exactly(prepared):
    hits = [info["ng"] == target for nlay in (54, 20) for target, info in _reproduce(prepared(nlay)[0], nlay)]
    assert len(hits) == 6 and sum(hits) >= 4, hits


def test_several_bands_with_different_tolerances(prepared):
    from ecckd_amd import api
    gases, _ = prepared(54)
    edges = [0, 9000, 21000, 34000, NWAV]
    given = np.array([0.08, 0.04, 0.08, 0.16])
    ng_offset = 4 * (1 - NGAS)
    _reset(gases)
    target = _total(api.find_g_gases(gases, [_req(0.55 * given, edges) for _ in gases], TOLTOL, ITER), ng_offset)
    _reset(gases)
    res, info = api.find_g_gases_target(gases, [_req(given, edges) for _ in gases], ng_offset, target, RESOLUTION, 40, TOLTOL, ITER)
    assert _total(res, ng_offset) == info["ng"]
    assert info["ng"] == target or (info["status"] == 1 and _straddled(info, target, RESOLUTION)), info
    for u in info["tolerance_used"]:
        assert u.dtype == np.float64 and u.tobytes() == (info["scaling"] * given).tobytes()
    _reset(gases)
    _same(res, api.find_g_gases(gases, [_req(info["tolerance_used"][k], edges) for k in range(NGAS)], TOLTOL, ITER))


def test_the_rerun_of_the_chosen_trial_comes_from_the_memo(prepared):
    """Two trials only, and a target one below what the first gives: the first trial is the answer but the second was the last
    one run, so the gases are searched once more at the first scaling - without a single point swept."""
    from ecckd_amd import api
    gases, _ = prepared(20)
    ng_offset = 1 - NGAS
    _reset(gases)
    n1 = _total(api.find_g_gases(gases, [_req(0.1) for _ in gases], TOLTOL, ITER), ng_offset)
    _reset(gases)
    swept = []
    res, info = api.find_g_gases_target(gases, [_req(0.1) for _ in gases], ng_offset, n1 - 1, RESOLUTION, 2, TOLTOL, ITER,
                                        on_trial=lambda i, s, n, per_gas: swept.append(sum(g.eval_stats()["points_evaluated"] for g in gases)))
    assert info["status"] == 2 and info["trials"][0] == (1.0, n1) and info["trials"][1][0] == 2.0 and len(swept) == 2
    assert abs(info["trials"][1][1] - (n1 - 1)) > 1, "the shapes of this test no longer force a re-run"
    assert (info["scaling"], info["ng"]) == info["trials"][0] and info["scaling"] != info["trials"][-1][0]
    after = sum(g.eval_stats()["points_evaluated"] for g in gases)
    assert swept[1] > swept[0] > 0 and after == swept[1]
    # the outputs are those of the chosen scaling, not of the last trial
    assert _total(res, ng_offset) == n1
    _reset(gases)
    _same(res, api.find_g_gases(gases, [_req(0.1) for _ in gases], TOLTOL, ITER))


def test_clamped_and_unreachable_targets(prepared):
    """max_g_points = 3 for each of the four gases: nine g points at the most, however tight the tolerance.  The first guess is
    loose (0.05 x 2^18) so that the twenty halvings down to 2^-20 end at a tolerance a search is normally run with."""
    from ecckd_amd import api
    gases, _ = prepared(20)
    ng_offset = 1 - NGAS
    clamp = [dict(max_g_points=3)]
    _reset(gases)
    res, info = api.find_g_gases_target(gases, [_req(0.05 * 2.0 ** 18, options=clamp) for _ in gases], ng_offset, 20, RESOLUTION, 40,
                                        TOLTOL, ITER)
    print("clamped:", info)
    assert info["status"] == 3 and [s for s, _ in info["trials"]] == [2.0 ** -k for k in range(21)]
    assert info["trials"][0][1] == 1 and info["ng"] == max(n for _, n in info["trials"]) <= 9 and info["ng"] >= 5
    assert _total(res, ng_offset) == info["ng"] and all(len(r["error"]) <= 3 for g_res in res for r in g_res)
    assert (info["scaling"], info["ng"]) in info["trials"]
    # below the minimum: every band of every gas has at least one g point, so the overlap has at least nband = 2
    edges = [0, 30000, NWAV]
    res, info = api.find_g_gases_target(gases, [_req(0.05, edges) for _ in gases], 2 * (1 - NGAS), 1, RESOLUTION, 40, TOLTOL, ITER)
    print("below the minimum:", info)
    assert info["status"] == 3 and [s for s, _ in info["trials"]] == [2.0 ** k for k in range(21)]
    assert info["ng"] == 2 and _total(res, 2 * (1 - NGAS)) == 2 and info["scaling"] == 2.0 ** 20


def test_refusals(prepared):
    from ecckd_amd import api, EcckdError
    gases, extra = prepared(20)
    ng_offset = 1 - NGAS
    before = [g.eval_stats() for g in gases]
    wn, rnk = extra[1]
    split = [dict(base_wn_bound=[0.0, 1000.0, 3261.0], wavenumber=wn, rank=rnk)]
    reqs = [_req(0.1) for _ in gases]
    with pytest.raises(EcckdError) as exc:
        api.find_g_gases_target(gases, [reqs[0], _req(0.1, options=split)] + reqs[2:], ng_offset, 12, RESOLUTION, 40, TOLTOL, ITER)
    assert exc.value.code == 147 and "request 1" in exc.value.message
    with pytest.raises(EcckdError) as exc:
        api.find_g_gases_target(gases, reqs, ng_offset, 0, RESOLUTION, 40, TOLTOL, ITER)
    assert exc.value.code == 147
    assert [g.eval_stats() for g in gases] == before            # refused before anything ran
    with pytest.raises(EcckdError) as exc:
        api.find_g_gases_target(gases, reqs, ng_offset, 2, RESOLUTION, 40, TOLTOL, ITER, trial_capacity=1)
    assert exc.value.code == 147 and "capacity" in exc.value.message
