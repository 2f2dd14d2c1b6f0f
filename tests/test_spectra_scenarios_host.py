"""The scenarios= argument of pipeline.lw_spectra / sw_spectra: every check of the tools' key fires as a ValueError before anything
touches a device (the api module is replaced by one that fails on any use, and the context is None), and the ctypes
signatures of the two new entry points are the prototypes of include/ecckd_hip.h.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"api.{name} used before the arguments were checked")


@pytest.fixture
def pipeline(monkeypatch):
    from ecckd_amd import ncio, pipeline
    monkeypatch.setattr(pipeline, "api", _NoDevice())
    monkeypatch.setattr(pipeline, "ncio", _NoDevice())
    assert ncio is not None
    return pipeline


def _lines(*outputs, n=2):
    return [dict(name=f"s{k}", output=o, scaling=[1.0] * n, conc=None) for k, o in enumerate(outputs)]


CASES = {
    "empty_table": (dict(scenarios=[]), "Scenario table is empty"),
    "output_beside": (dict(scenarios=_lines("a.nc"), output_path="o.nc"), '"output_path" cannot be combined with "scenarios"'),
    "scaling_beside": (dict(scenarios=_lines("a.nc"), scaling=[1.0, 1.0]), '"scaling" cannot be combined with "scenarios"'),
    "conc_beside": (dict(scenarios=_lines("a.nc"), conc=[1e-3, -1]), '"conc" cannot be combined with "scenarios"'),
    "too_few_scalings": (dict(scenarios=_lines("a.nc") + [dict(name="b", output="b.nc", scaling=[2.0])]),
                         "scenario 2: 1 scaling value(s) for 2 spectrum file(s)"),
    "too_many_concs": (dict(scenarios=[dict(name="b", output="b.nc", conc=[1e-3, -1, -1])]), "scenario 1: 3 conc value(s) for 2 spectrum file(s)"),
    "const": (dict(scenarios=[dict(name="b", output="b.nc", const=[1e-3, 1e-3])]), "const=C is not a scaling"),
    "unknown_spec": (dict(scenarios=[dict(name="b", output="b.nc", double=[2, 2])]), "unknown scaling spec ['double']"),
    "duplicate_output": (dict(scenarios=_lines("a.nc", "a.nc")), 'scenario 2: duplicate output file "a.nc"'),
    "output_is_an_input": (dict(scenarios=_lines("a.nc", "co2.nc")), 'the output "co2.nc" is the input file of this run'),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("sw", [False, True], ids=["lw_spectra", "sw_spectra"])
def test_checks_fire_before_the_device(pipeline, case, sw):
    kw, message = CASES[case]
    with pytest.raises(ValueError) as e:
        if sw:
            pipeline.sw_spectra(None, ["h2o.nc", "co2.nc"], None, **kw)
        else:
            pipeline.lw_spectra(None, ["h2o.nc", "co2.nc"], **kw)
    assert message in str(e.value)


def test_more_than_sixteen_inputs_and_the_rayleigh_file(pipeline):
    with pytest.raises(ValueError) as e:
        pipeline.lw_spectra(None, ["h2o.nc"] * 17, scenarios=_lines("a.nc", n=17))
    assert "17 input files, 16 at most" in str(e.value)
    with pytest.raises(ValueError) as e:
        pipeline.sw_spectra(None, ["h2o.nc", "co2.nc"], None, rayleigh="ray.nc", scenarios=_lines("a.nc", "ray.nc"))
    assert 'the output "ray.nc" is the rayleigh file of this run' in str(e.value)
    with pytest.raises(ValueError):
        pipeline.lw_spectra(None, [], scenarios=_lines("a.nc", n=0))


def test_accepted_table(pipeline):
    """None in a list is "as the file holds it"; an entry without output is computed and not written"""
    table = pipeline._check_scenarios([dict(name="a", output=None, scaling=[None, 2], conc=None), dict(name="b", output="b.nc", conc=[1e-3, None])],
                                      ["h2o.nc", "co2.nc"], {"rayleigh": None}, output_path=None, scaling=None, conc=None)
    assert table == [("a", None, [-1.0, 2.0], None), ("b", "b.nc", None, [1e-3, -1.0])]


CTYPE = {"int": C.c_int, "size_t": C.c_size_t, "ecckd_ctx*": C.c_void_p, "const void* const*": C.POINTER(C.c_void_p), "const int*": C.POINTER(C.c_int),
         "const size_t*": C.POINTER(C.c_size_t), "const double*": C.POINTER(C.c_double), "double*": C.c_void_p, "int*": C.POINTER(C.c_int)}


@pytest.mark.parametrize("name", ["ecckd_merge_scenario_dev", "ecckd_merge_scenario_geometry"])
def test_ctypes_signature_is_the_headers(name):
    """argument by argument; h_scale is a host array (a ctypes double pointer), d_merged a device address (void pointer)"""
    from ecckd_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ecckd_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name
    args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in m.group(1).split(",")]      # the type: all but the name
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == len(args), (args, argtypes)
    for text, got in zip(args, argtypes):
        assert CTYPE[text] is got or CTYPE[text] == got, (name, text, got)
