"""The search for the tolerance scaling that yields a wanted number of g points (ecckd_target_search), through the library,
on count functions whose answers are known trial by trial.  CPU only: the search is host code; the GPU enters only through
the count callback (ecckd_find_g_gases_target)."""
import math

import pytest

PARAMETER_ERROR, PROCESSING_ERROR = 147, 148


def _f32(s):
    return int(math.floor(32.0 / s))


def _best(trials, target):
    """Step 4 of the algorithm: smallest |ng - target|, among equals ng < target, then the larger scaling."""
    return min(trials, key=lambda t: (abs(t[1] - target), 0 if t[1] < target else 1, -t[0]))


def test_target_met_while_bracketing():
    from ecckd_amd import api
    r = api.target_search(_f32, 8)
    assert r["trials"] == [(1.0, 32), (2.0, 16), (4.0, 8)]
    assert (r["status"], r["scaling"], r["ng"]) == (0, 4.0, 8)
    r = api.target_search(_f32, 32)
    assert r["trials"] == [(1.0, 32)] and (r["status"], r["scaling"], r["ng"]) == (0, 1.0, 32)


def test_bisection_trial_by_trial():
    from ecckd_amd import api
    r = api.target_search(_f32, 10)
    s3 = math.sqrt(2.0 * 4.0)
    s4 = math.sqrt(s3 * 4.0)
    s5 = math.sqrt(s3 * s4)
    assert [t[0] for t in r["trials"]] == [1.0, 2.0, 4.0, s3, s4, s5]          # the same doubles
    assert [t[1] for t in r["trials"]] == [32, 16, 8, 11, 9, 10]
    assert (r["status"], r["scaling"], r["ng"]) == (0, s5, 10)


def test_downwards():
    from ecckd_amd import api
    r = api.target_search(_f32, 100)
    assert r["trials"][:3] == [(1.0, 32), (0.5, 64), (0.25, 128)]
    # the bisection follows: lo = 1/4 (128 > 100), hi = 1/2 (64 < 100)
    lo, hi = 0.25, 0.5
    for s, n in r["trials"][3:]:
        assert s == math.sqrt(lo * hi) and n == _f32(s)
        if n > 100:
            lo = s
        elif n < 100:
            hi = s
    assert (r["status"], r["ng"]) == (0, 100) and r["trials"][-1] == (r["scaling"], 100)
    assert _f32(r["scaling"]) == 100


@pytest.mark.parametrize("resolution", [1e-3, 1e-6])
def test_a_function_that_jumps_over_the_target(resolution):
    """12 g points up to s = 2.5, 8 above: a target of 10 (or of 9 or 11) cannot be met."""
    from ecckd_amd import api
    fn = lambda s: 12 if s <= 2.5 else 8        # noqa: E731
    for target, want in ((10, 8), (11, 12), (9, 8)):
        r = api.target_search(fn, target, resolution=resolution, max_trials=60)
        assert r["status"] == 1
        assert (r["scaling"], r["ng"]) == _best(r["trials"], target) and r["ng"] == want
        above = [s for s, n in r["trials"] if n > target]       # lo: the largest scaling that gave more
        below = [s for s, n in r["trials"] if n < target]
        lo, hi = max(above), min(below)
        assert lo <= 2.5 < hi and hi / lo <= 1.0 + resolution
        assert (lo, 12) in r["trials"] and (hi, 8) in r["trials"]
        # among equals (target 10: 12 and 8 are both 2 away) the one below the target, and of those the larger scaling
        if target == 10:
            assert r["scaling"] == max(below)


def test_plateau_and_max_trials():
    from ecckd_amd import api
    fn = lambda s: min(_f32(s), 20)             # noqa: E731
    r = api.target_search(fn, 25)
    assert r["status"] == 3 and r["ng"] == 20
    assert [t[0] for t in r["trials"]] == [2.0 ** -k for k in range(21)]        # never below 2^-20
    assert r["scaling"] == 1.0                                                   # among equals the larger scaling
    r = api.target_search(fn, 25, max_trials=5)
    assert r["status"] == 2 and len(r["trials"]) == 5 and r["ng"] == 20
    # upwards: at least one g point however large the scaling
    r = api.target_search(lambda s: max(_f32(s), 3), 2)
    assert r["status"] == 3 and r["ng"] == 3 and r["trials"][-1][0] == 2.0 ** 20 and r["scaling"] == 2.0 ** 20
    # max_trials spent in the bisection
    r = api.target_search(lambda s: 12 if s <= 2.5 else 8, 10, resolution=1e-9, max_trials=7)
    assert r["status"] == 2 and len(r["trials"]) == 7
    assert (r["scaling"], r["ng"]) == _best(r["trials"], 10)


def test_non_monotone_function():
    from ecckd_amd import api
    calls = []

    def fn(s):
        calls.append(s)
        return int(40.0 / s + 6.0 * math.sin(37.0 * s))

    for target in (7, 13, 25, 90):
        del calls[:]
        r = api.target_search(fn, target, resolution=1e-4, max_trials=40)
        assert r["status"] in (0, 1, 2)
        assert [t[0] for t in r["trials"]] == calls and len(calls) <= 40
        assert (r["scaling"], r["ng"]) == _best(r["trials"], target)
        assert (r["status"] == 0) == (r["ng"] == target)


def test_refusals():
    from ecckd_amd import api, EcckdError
    for kw in (dict(target=0), dict(target=8, resolution=0.0), dict(target=8, resolution=-1.0), dict(target=8, max_trials=0)):
        with pytest.raises(EcckdError) as exc:
            api.target_search(_f32, **kw)
        assert exc.value.code == PARAMETER_ERROR and exc.value.message
    with pytest.raises(EcckdError) as exc:
        api.target_search(None, 8)
    assert exc.value.code == PARAMETER_ERROR and "fn" in exc.value.message


def test_callback_error_and_overflowing_trial_list():
    from ecckd_amd import api, EcckdError

    def fails_third(s):
        if s == 4.0:
            raise EcckdError(PROCESSING_ERROR, "no such count")
        return _f32(s)

    with pytest.raises(EcckdError) as exc:
        api.target_search(fails_third, 5)
    assert exc.value.code == PROCESSING_ERROR and "4" in exc.value.message
    # six trials are needed for 10 g points: five slots overflow, six do not
    with pytest.raises(EcckdError) as exc:
        api.target_search(_f32, 10, capacity=5)
    assert exc.value.code == PARAMETER_ERROR and "capacity" in exc.value.message
    assert api.target_search(_f32, 10, capacity=6)["status"] == 0
